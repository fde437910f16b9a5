"""The blend outputs through the C++ twin (Engine::SetBatchBlends, host.py's blends= / blend_gain= arguments): a one-shard engine's one-call
run and its streamed job write N + 3 + B files whose blend ports are the restatements (tests/blend_ref.py, tests/trim_ref.py) of the call's
own chain rows, with ports 0 .. N + 2 those of the engine without blends; every record list has N + 3 + B ports; render_normalized plans
a blend port's gain from its own true-peak records; an engine of two shards refuses, and says why."""
import numpy as np
import pytest

import blend_ref
import trim_ref
from test_host_mirror_batch_dither import _inputs
import __graft_entry__ as entry
from test_host_mirror_batch_stream import BLOCK, _engine

pytestmark = pytest.mark.gpu

SEED = 0x3c9a1f5e7b2d4680
BLENDS = [[(0, 1.0)], [(0, 0.6), (1, 0.4)], [(2, -1.0), (0, 0.1), (1, 0.2), (2, 0.3)]]
GAIN = [0.5, -1.7, 1.0]


@pytest.fixture(scope="module")
def host():
    entry.load_package()                                                 # build() has made both libraries
    from go_dsp_guitar_amd import host as h
    return h


def test_a_one_shard_engine_writes_the_blend_ports_and_leaves_the_others(host):
    sr, nch = 48000, 3
    no, nb = nch + 3, len(BLENDS)
    inputs = _inputs(sr, nch)
    kw = dict(window=2, metronome_to_master=True)
    runs, peaks = {}, {}
    for name, fmt, blends, gain, dither in (("rows", "ieee64", BLENDS, None, None), ("off", "lpcm24", None, None, SEED), ("on", "lpcm24", BLENDS, GAIN, SEED),
                                            ("streamed", "lpcm24", BLENDS, GAIN, SEED)):
        eng, sp = _engine(host, nch, sr)                                 # a fresh engine per job: the units start from rest
        if name == "streamed":
            it = iter([1, 2])
            parts = list(eng.batch_stream(inputs, sr, fmt, lambda left: next(it), dither=dither, blends=blends, blend_gain=gain, true_peak=True, **kw))
            runs[name] = [np.concatenate([p[r] for p in parts]) for r in range(no + nb)]
        else:
            runs[name] = [o.copy() for o in eng.batch_run(inputs, sr, fmt, dither=dither, blends=blends, blend_gain=gain, report=True, true_peak=True, **kw)]
            assert eng.last_report.shape[0] == len(runs[name])
        peaks[name] = eng.last_true_peak.copy()
        assert eng.last_error() == "" and len(runs[name]) == (no if blends is None else no + nb)
        del sp
        eng.close()
    rows = [o.view(np.float64) for o in runs["rows"]]
    want = blend_ref.blends(np.stack(rows[:nch]), BLENDS)
    for b in range(nb):
        assert blend_ref.same_bits(rows[no + b], want[b]), b
        enc = trim_ref.encode("lpcm24", rows[no + b], GAIN[b], SEED, no + b, 0)
        assert np.array_equal(runs["on"][no + b], enc), "blend %d" % b
    for r in range(no):                                                  # the engine without blends goes through the shard calls and the finish: the same files
        assert np.array_equal(runs["on"][r], runs["off"][r]), r
    for r in range(no + nb):
        assert np.array_equal(runs["streamed"][r], runs["on"][r]), "streamed, output %d" % r
    assert peaks["on"].shape == (no + nb, 3) and peaks["on"][:no].tobytes() == peaks["off"].tobytes()
    assert peaks["streamed"].tobytes() == peaks["on"].tobytes() and peaks["on"][no:].tobytes() == peaks["rows"][no:].tobytes()      # before the gain


def test_render_normalized_plans_the_gain_of_a_blend_port_from_its_own_records(host):
    pkg = entry.load_package()
    sr, nch = 48000, 3
    no, nb = nch + 3, len(BLENDS)
    inputs = _inputs(sr, nch)
    eng, sp = _engine(host, nch, sr)
    rows = [o.view(np.float64).copy() for o in eng.batch_run(inputs, sr, "ieee64", window=2, blends=BLENDS)]
    del sp
    eng.close()
    eng, sp = _engine(host, nch, sr)
    outs, gains = eng.render_normalized(-1.0, 40.0, inputs, sr, "lpcm24", window=2, blends=BLENDS, blend_gain=[9.0, 9.0, 9.0])
    assert len(outs) == no + nb and gains.shape == (no + nb,) and eng.normalize_true_peak.shape[0] == no + nb
    assert np.array_equal(gains, pkg.trim_from_true_peak(eng.normalize_true_peak, 10.0 ** (-1.0 / 20.0), 10.0 ** (40.0 / 20.0)))
    for b in range(nb):
        assert gains[no + b] != 1.0 and gains[no + b] != 9.0
        assert np.array_equal(outs[no + b], trim_ref.encode("lpcm24", rows[no + b], gains[no + b])), "blend %d" % b
    del sp
    eng.close()


def test_two_shards_refuse_and_a_refused_list_leaves_the_one_in_force(host):
    sr, nch = 48000, 4
    inputs = _inputs(sr, nch, blocks=1)
    eng, sp = _engine(host, nch, sr, devices=[0, 0])
    with pytest.raises(host.HostError, match="2 shards.*holds its own channels only"):
        eng.batch_run(inputs, sr, "lpcm16", blends=BLENDS)
    del sp
    eng.close()
    eng, sp = _engine(host, nch, sr)
    assert eng._set_blends(BLENDS, GAIN) == 3
    for blends, gain, what in (([[(0, 1.0)], [(4, 1.0)]], None, "blend 1, term 0"), ([[(0, 1.0)], []], None, "blend 1 has 0 terms"),
                               ([[(0, 1.0)] * 33], None, "33 terms"), ([[(0, float("inf"))]], None, "blend 0, term 0"), ([[(0, 1.0)]], [float("nan")], "gain")):
        with pytest.raises(host.HostError, match=what):
            eng._set_blends(blends, gain)
        assert host.lib().gdgh_engine_batch_blends(eng._h) == 3
    assert eng._set_blends(None) == 0
    del sp
    eng.close()
