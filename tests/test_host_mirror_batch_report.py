"""The render report through the C++ twin (Engine::SetBatchReport / LastBatchReport, host.py's report=True): last_report is [N + 3, blocks]
in the plain run's port order whatever the shard count -- chain rows from the shards' reports side by side, the master from the finish,
the metronome from the shard that ran it.  IEEE64 files hold the pre-encode samples (wave.go:694-709: no clamp), so every record is
checked against numpy on the engine's own output; chain and metronome rows are byte-equal across shard counts and slicings."""
import numpy as np
import pytest

from test_gpu_block_stats import check_records, ref_stats
from test_host_mirror_batch_stream import BLOCK, _engine, _files, host  # noqa: F401 (host: the module's fixture)

pytestmark = pytest.mark.gpu


def test_engine_reports_the_plain_order_whatever_the_shard_count(host, oracle):
    sr, nch = 48000, 4
    inputs = _files(oracle, sr)
    eng, sp = _engine(host, nch, sr)
    outs = eng.batch_run(inputs, sr, "ieee64", window=4, metronome_to_master=True)
    assert eng.last_report is None, "off by default"
    with pytest.raises(host.HostError, match="no report"):
        eng._fetch("report")
    del sp
    eng.close()
    eng, sp = _engine(host, nch, sr)
    outs_on = eng.batch_run(inputs, sr, "ieee64", window=4, metronome_to_master=True, report=True)
    one = eng.last_report
    del sp
    eng.close()
    assert [o.tobytes() for o in outs_on] == [o.tobytes() for o in outs], "the report changes no output byte"
    blocks = outs[0].size // 8 // BLOCK
    assert one.shape == (nch + 3, blocks) and blocks >= 8
    check_records(one, np.stack([ref_stats(o.view(np.float64), BLOCK) for o in outs_on]), BLOCK, "Engine.batch_run")
    assert tuple(one[2, 0]) == (0.0, 0.0, 0, 0, 0, 0) and one["peak"][nch + 2].max() > 0        # the empty channel; the metronome
    # a one-shard engine's plain streamed run: the same records, slice by slice
    eng, sp = _engine(host, nch, sr)
    parts = list(eng.batch_stream(inputs, sr, "ieee64", 3, window=4, metronome_to_master=True, report=True))
    assert eng.last_report.shape == one.shape
    dec = [np.concatenate([p[r] for p in parts]).view(np.float64) for r in range(nch + 3)]
    check_records(eng.last_report, np.stack([ref_stats(d, BLOCK) for d in dec]), BLOCK, "Engine.batch_stream")
    keep = list(range(nch)) + [nch + 2]
    assert eng.last_report[keep].tobytes() == one[keep].tobytes()
    del sp
    eng.close()
    for devices in ([0, 0], [0, 0, 0]):
        eng, sp = _engine(host, nch, sr, devices=devices)
        it = iter([1, 4, blocks - 5])
        parts = list(eng.batch_stream_sharded(inputs, sr, "ieee64", lambda left: next(it), window=4, metronome_to_master=True, report=True))
        got = eng.last_report
        assert eng.last_error() == "" and got.shape == one.shape
        assert got[keep].tobytes() == one[keep].tobytes(), "chain outputs and metronome, %d shards" % len(devices)
        dec = [np.concatenate([p[r] for p in parts]).view(np.float64) for r in range(nch + 3)]
        check_records(got, np.stack([ref_stats(d, BLOCK) for d in dec]), BLOCK, "Engine.batch_stream_sharded, %d shards" % len(devices))
        got_run = eng.batch_run(inputs, sr, "ieee64", window=4, metronome_to_master=True, report=True)
        check_records(eng.last_report, np.stack([ref_stats(o.view(np.float64), BLOCK) for o in got_run]), BLOCK, "Engine.batch_run, %d shards" % len(devices))
        del sp
        eng.close()
