"""The alignment report through the C++ twin (Engine::SetBatchAlign / LastBatchAlign, host.py's align=(ref, max_lag)): last_align is
[N + 3, blocks] in the plain run's port order whatever the shard count -- chain rows from the shards side by side, the metronome from
shard 0, the master rows zero records over the shard forms (the finish carries none).  The single context's records (a one-shard engine's
plain streamed run, which is gdg_batch_stream_step on one context) are the reference: chain and metronome rows equal them on the bytes
over 1 and 2 shards.  A reference across shards and a master port in a sharded list are refused."""
import numpy as np
import pytest

from test_host_mirror_batch_stream import BLOCK, _engine, _files, host  # noqa: F401 (host: the module's fixture)

pytestmark = pytest.mark.gpu

M = 64


def test_engine_keeps_the_plain_order_whatever_the_shard_count(host, oracle):
    sr, nch = 48000, 4
    inputs = _files(oracle, sr)
    kw = dict(window=4, metronome_to_master=True)
    # two shards hold channels 0, 1 and 2, 3: every chain port against the first channel of its shard, the metronome against itself
    ref = [0, 0, 2, 2, -1, -1, nch + 2]
    with_master = [0, 0, 2, 2, 0, nch, nch + 2]
    # the single context: a one-shard engine's plain streamed run, to IEEE64 (the files are the rows), the master measured too
    eng, sp = _engine(host, nch, sr)
    parts = list(eng.batch_stream(inputs, sr, "ieee64", 3, align=(with_master, M), **kw))
    one = eng.last_align
    rows = np.stack([np.concatenate([p[r] for p in parts]).view(np.float64) for r in range(nch + 3)])
    blocks = rows.shape[1] // BLOCK
    assert eng.last_error() == "" and one.shape == (nch + 3, blocks) and one.dtype.itemsize == 40 and blocks >= 8
    assert one.tobytes() == eng.raw_context(0).block_align(rows, with_master, M).tobytes()
    # channel 0 against itself, over the three blocks its 30000 input samples fill: no shift.  (Behind them the block holds the chain's
    # decaying tail, and the reference's central slice meets the louder samples in front of it: the greatest |r| lies at -M, by the definition.)
    full = one[0][:3]
    assert np.all(full["lag"] == 0) and np.all(np.abs(full["corr"] - full["ref_sq"]) <= 1e-12 * full["ref_sq"]) and np.all(full["corr"] == full["corr0"])
    assert np.any(one[nch]["ref_sq"] > 0.0)
    del sp
    eng.close()
    # off by default
    eng, sp = _engine(host, nch, sr)
    plain = eng.batch_run(inputs, sr, "lpcm24", **kw)
    assert eng.last_align is None
    with pytest.raises(host.HostError, match="no alignment records"):
        eng._fetch("align")
    # the shard forms make the master in the finish: a list that touches it is refused when the job is set up, at any shard count
    with pytest.raises(host.HostError, match="master mix"):
        eng.batch_run(inputs, sr, "lpcm24", align=(with_master, M), **kw)
    del sp
    eng.close()
    keep = list(range(nch)) + [nch + 2]
    for devices in (None, [0, 0]):
        n = 1 if devices is None else len(devices)
        eng, sp = _engine(host, nch, sr, devices=devices)
        outs = eng.batch_run(inputs, sr, "lpcm24", align=(ref, M), **kw)
        got = eng.last_align
        assert eng.last_error() == "" and got.shape == (nch + 3, blocks), n
        assert got[keep].tobytes() == one[keep].tobytes(), "Engine.batch_run, %d shard(s): chain outputs and metronome" % n
        assert got[nch:nch + 2].tobytes() == bytes(40 * 2 * blocks), "the master rows are zero records"
        assert [o.tobytes() for o in outs] == [o.tobytes() for o in plain], "the alignment report changes no output byte"
        del sp
        eng.close()
        eng, sp = _engine(host, nch, sr, devices=devices)
        it = iter([1, 4, blocks - 5])
        list(eng.batch_stream_sharded(inputs, sr, "lpcm24", lambda left: next(it), report=True, align=(ref, M), **kw))
        got = eng.last_align
        assert eng.last_error() == "" and eng.last_report.shape == (nch + 3, blocks) and got.shape == (nch + 3, blocks)
        assert got[keep].tobytes() == one[keep].tobytes() and got[nch:nch + 2].tobytes() == bytes(40 * 2 * blocks), "Engine.batch_stream_sharded, %d shard(s)" % n
        del sp
        eng.close()
    # two shards: a reference across shards and a master port are refused, and the engine stays as it was
    eng, sp = _engine(host, nch, sr, devices=[0, 0])
    with pytest.raises(host.HostError, match="live on one shard"):
        eng.batch_run(inputs, sr, "lpcm24", align=([0, 0, 0, 2, -1, -1, -1], M), **kw)
    with pytest.raises(host.HostError, match="live on one shard"):
        eng.batch_run(inputs, sr, "lpcm24", align=([0, 0, nch + 2, 2, -1, -1, -1], M), **kw)     # the metronome lives on shard 0
    with pytest.raises(host.HostError, match="master mix"):
        eng.batch_run(inputs, sr, "lpcm24", align=(with_master, M), **kw)
    with pytest.raises(host.HostError, match="lag range"):
        eng.batch_run(inputs, sr, "lpcm24", align=(ref, 4096), **kw)
    outs = eng.batch_run(inputs, sr, "lpcm24", align=(ref, M), **kw)
    assert eng.last_align[keep].tobytes() == one[keep].tobytes() and [o.tobytes() for o in outs] == [o.tobytes() for o in plain]
    del sp
    eng.close()
