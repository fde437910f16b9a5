"""The true-peak records through the C++ twin (Engine::SetBatchTruePeak / LastBatchTruePeak, host.py's true_peak=True): last_true_peak is
[N + 3, blocks] in the plain run's port order whatever the shard count -- chain rows from the shards side by side, the master's two from
the finish, the metronome from shard 0.  The single context's records (a one-shard engine's plain streamed run, which is
gdg_batch_stream_step on one context) are the reference: chain and metronome rows equal them on the bytes over 1 and 2 shards; the master
rows, whose sums the finish associates differently, agree within 1e-12 relative, with the position equal wherever the restatement's
runner-up stands 1 % below the maximum."""
import numpy as np
import pytest

import true_peak_ref as ref
from test_host_mirror_batch_stream import BLOCK, _engine, _files, host  # noqa: F401 (host: the module's fixture)

pytestmark = pytest.mark.gpu


def test_engine_keeps_the_plain_order_whatever_the_shard_count(host, oracle):
    sr, nch = 48000, 4
    inputs = _files(oracle, sr)
    kw = dict(window=4, metronome_to_master=True)
    # the single context: a one-shard engine's plain streamed run, to IEEE64 (the files are the rows)
    eng, sp = _engine(host, nch, sr)
    parts = list(eng.batch_stream(inputs, sr, "ieee64", 3, true_peak=True, **kw))
    one = eng.last_true_peak
    rows = np.stack([np.concatenate([p[r] for p in parts]).view(np.float64) for r in range(nch + 3)])
    blocks = rows.shape[1] // BLOCK
    assert eng.last_error() == "" and one.shape == (nch + 3, blocks) and one.dtype.itemsize == 16 and blocks >= 8
    raw = eng.raw_context(0)
    assert one.tobytes() == raw.block_true_peak(rows).tobytes()
    import __graft_entry__ as entry
    taps = entry.load_package().true_peak_taps()
    assert one.tobytes() == ref.block_true_peak(rows, taps).tobytes()
    assert np.any(one["true_peak"][nch] > 0.0)
    del sp
    eng.close()
    # off by default
    eng, sp = _engine(host, nch, sr)
    plain = eng.batch_run(inputs, sr, "lpcm24", **kw)
    assert eng.last_true_peak is None
    with pytest.raises(host.HostError, match="no true-peak records"):
        eng._fetch("true_peak")
    del sp
    eng.close()
    keep = list(range(nch)) + [nch + 2]

    def check(got, what):
        assert got.shape == (nch + 3, blocks), what
        assert got[keep].tobytes() == one[keep].tobytes(), "%s: chain outputs and metronome" % what
        for s in (nch, nch + 1):
            assert np.all(np.abs(got[s]["true_peak"] - one[s]["true_peak"]) <= 1e-12 * one[s]["true_peak"]), "%s: master row %d" % (what, s)
            for b in range(blocks):
                if ref.runner_up(rows[s][b * BLOCK:(b + 1) * BLOCK], taps) <= 0.99:
                    assert got[s][b]["position"] == one[s][b]["position"], (what, s, b)

    for devices in (None, [0, 0]):
        n = 1 if devices is None else len(devices)
        eng, sp = _engine(host, nch, sr, devices=devices)
        outs = eng.batch_run(inputs, sr, "lpcm24", true_peak=True, **kw)
        assert eng.last_error() == ""
        check(eng.last_true_peak, "Engine.batch_run, %d shard(s)" % n)
        assert [o.tobytes() for o in outs] == [o.tobytes() for o in plain], "the true peak changes no output byte"
        del sp
        eng.close()
        eng, sp = _engine(host, nch, sr, devices=devices)
        it = iter([1, 4, blocks - 5])
        list(eng.batch_stream_sharded(inputs, sr, "lpcm24", lambda left: next(it), report=True, true_peak=True, **kw))
        assert eng.last_error() == "" and eng.last_report.shape == (nch + 3, blocks)
        check(eng.last_true_peak, "Engine.batch_stream_sharded, %d shard(s)" % n)
        assert np.all(eng.last_true_peak["true_peak"] >= eng.last_report["peak"])
        del sp
        eng.close()
