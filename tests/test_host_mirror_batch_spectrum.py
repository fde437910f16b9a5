"""The band spectrum through the C++ twin (Engine::SetBatchSpectrum / LastBatchSpectrum, host.py's spectrum=edges): last_spectrum is
[N + 3, blocks, bands] in the plain run's port order whatever the shard count -- chain rows from the shards side by side, the master
from the finish, the metronome from shard 0.  The single context's bands (a one-shard engine's plain streamed run, which is
gdg_batch_stream_step on one context) are the reference: chain and metronome rows equal them on the bytes over 1 and 2 shards, the
master -- whose sums the finish associates differently -- within 1e-12 * T, T = the numpy restatement's sum over all bins of the block."""
import numpy as np
import pytest

import spectrum_ref as ref
from test_host_mirror_batch_stream import BLOCK, _engine, _files, host  # noqa: F401 (host: the module's fixture)

pytestmark = pytest.mark.gpu

EDGES = [22.1 * 2.0 ** i for i in range(10)] + [24000.0, 30000.0]


def test_engine_keeps_the_plain_order_whatever_the_shard_count(host, oracle):
    sr, nch = 48000, 4
    inputs = _files(oracle, sr)
    kw = dict(window=4, metronome_to_master=True)
    # the single context: a one-shard engine's plain streamed run, to IEEE64 (the files are the rows) ...
    eng, sp = _engine(host, nch, sr)
    parts = list(eng.batch_stream(inputs, sr, "ieee64", 3, spectrum=EDGES, **kw))
    one = eng.last_spectrum
    rows = np.stack([np.concatenate([p[r] for p in parts]).view(np.float64) for r in range(nch + 3)])
    blocks = rows.shape[1] // BLOCK
    assert eng.last_error() == "" and one.shape == (nch + 3, blocks, len(EDGES) - 1) and blocks >= 8
    # ... whose bands are the stand-alone entry's on those rows, and the restatement's within the bound
    assert one.tobytes() == eng.raw_context(0).block_spectrum(rows, sr, EDGES).tobytes()
    tot = np.stack([ref.block_spectrum(r, sr, EDGES)[1] for r in rows])
    for r in range(nch + 3):
        assert np.all(np.abs(one[r] - ref.block_spectrum(rows[r], sr, EDGES)[0]) <= 1e-12 * tot[r][:, None]), r
    assert np.all(one[2] == 0.0) and one[nch + 2].sum() > 0.0         # the empty channel; the metronome
    del sp
    eng.close()
    # off by default, and off again
    eng, sp = _engine(host, nch, sr)
    plain = eng.batch_run(inputs, sr, "lpcm24", **kw)
    assert eng.last_spectrum is None
    with pytest.raises(host.HostError, match="no spectrum"):
        eng._fetch("spectrum")
    del sp
    eng.close()
    keep = list(range(nch)) + [nch + 2]

    def check(got, what):
        assert got.shape == one.shape, what
        assert got[keep].tobytes() == one[keep].tobytes(), "%s: chain outputs and metronome" % what
        for side in (nch, nch + 1):
            assert np.all(np.abs(got[side] - one[side]) <= 1e-12 * tot[side][:, None]), "%s: master row %d" % (what, side)

    for devices in (None, [0, 0]):
        n = 1 if devices is None else len(devices)
        eng, sp = _engine(host, nch, sr, devices=devices)
        outs = eng.batch_run(inputs, sr, "lpcm24", spectrum=EDGES, **kw)
        assert eng.last_error() == ""
        check(eng.last_spectrum, "Engine.batch_run, %d shard(s)" % n)
        assert [o.tobytes() for o in outs] == [o.tobytes() for o in plain], "the spectrum changes no output byte"
        del sp
        eng.close()
        eng, sp = _engine(host, nch, sr, devices=devices)
        it = iter([1, 4, blocks - 5])
        list(eng.batch_stream_sharded(inputs, sr, "lpcm24", lambda left: next(it), report=True, spectrum=EDGES, **kw))
        assert eng.last_error() == "" and eng.last_report.shape == (nch + 3, blocks)
        check(eng.last_spectrum, "Engine.batch_stream_sharded, %d shard(s)" % n)
        del sp
        eng.close()
    # a refused list leaves the engine as it was
    eng, sp = _engine(host, nch, sr)
    with pytest.raises(host.HostError, match="edge 1"):
        eng.batch_run(inputs, sr, "lpcm24", spectrum=[100.0, 50.0], **kw)
    del sp
    eng.close()
