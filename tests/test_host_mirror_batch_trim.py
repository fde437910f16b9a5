"""The output trim through the C++ twin (Engine::SetBatchTrim, host.py's trim= argument): the engine gives every shard its own slice of
the job's chain gains and the finishing context the master's, so a two-shard job writes the chain and metronome files of the one-shard
job byte for byte -- each the restatement (tests/trim_ref.py) of the job's float64 rows -- and its master is the restatement of the
finish's own sums; the streamed sharded job writes the one-call job's files; the records stay those of the render."""
import numpy as np
import pytest

import trim_ref as ref
from test_host_mirror_batch_dither import _inputs
import __graft_entry__ as entry
from test_host_mirror_batch_stream import BLOCK, _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    entry.load_package()                                                 # build() has made both libraries
    from go_dsp_guitar_amd import host as h
    return h


def test_every_shard_gets_its_gains_and_the_finish_the_master_s(host):
    sr, nch = 48000, 4
    inputs = _inputs(sr, nch)
    gains = np.array([0.5, -1.0, 1.7, 0.25, 0.8, -0.6, 3.0])             # four chains (two per shard), master left, master right, metronome
    kw = dict(window=2, metronome_to_master=True)
    runs, reports = {}, {}
    for name, devices, fmt, trim in (("one", None, "lpcm24", gains), ("rows", None, "ieee64", None), ("two", [0, 0], "lpcm24", gains),
                                     ("two, rows", [0, 0], "ieee64", None), ("two, streamed", [0, 0], "lpcm24", gains), ("two, off", [0, 0], "lpcm24", None)):
        eng, sp = _engine(host, nch, sr, devices=devices)                # a fresh engine per job: the units start from rest
        if name == "two, streamed":
            it = iter([1, 2])
            parts = list(eng.batch_stream_sharded(inputs, sr, fmt, lambda left: next(it), trim=trim, **kw))
            runs[name] = [np.concatenate([p[r] for p in parts]) for r in range(nch + 3)]
        else:
            runs[name] = [o.copy() for o in eng.batch_run(inputs, sr, fmt, trim=trim, report=True, true_peak=True, **kw)]
            reports[name] = (eng.last_report.tobytes(), eng.last_true_peak.tobytes())
        assert eng.last_error() == ""
        del sp
        eng.close()
    rows, rows2 = [o.view(np.float64) for o in runs["rows"]], [o.view(np.float64) for o in runs["two, rows"]]
    for r in list(range(nch)) + [nch + 2]:                               # chains and metronome: the same rows on one shard and on two
        want = ref.encode("lpcm24", rows[r], gains[r])
        assert np.array_equal(runs["one"][r], want), "one shard, output %d" % r
        assert np.array_equal(runs["two"][r], want), "two shards, output %d" % r
        assert not np.array_equal(runs["two"][r], runs["two, off"][r]), r
    for r in (nch, nch + 1):                                             # the master: each engine's own sums
        assert np.array_equal(runs["one"][r], ref.encode("lpcm24", rows[r], gains[r])), "one shard, master %d" % r
        assert np.array_equal(runs["two"][r], ref.encode("lpcm24", rows2[r], gains[r])), "two shards, master %d" % r
    for r in range(nch + 3):
        assert np.array_equal(runs["two, streamed"][r], runs["two"][r]), "streamed, output %d" % r
    assert reports["two"] == reports["two, off"] and reports["two"] == reports["two, rows"]          # the records describe the render, before the trim


def test_a_refused_list_leaves_the_gains_in_force(host):
    sr, nch = 48000, 2
    inputs = _inputs(sr, nch, blocks=1)
    eng, sp = _engine(host, nch, sr)
    with pytest.raises(host.HostError, match="gains"):
        eng.batch_run(inputs, sr, "lpcm16", trim=[0.5, 0.5, 1.0])       # N + 3 = 5
    with pytest.raises(host.HostError, match="not finite"):
        eng.batch_run(inputs, sr, "lpcm16", trim=[0.5, float("nan"), 1.0, 1.0, 1.0])
    assert eng.last_error() == ""
    del sp
    eng.close()
