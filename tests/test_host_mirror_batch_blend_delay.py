"""A delay per blend term through the C++ twin (Engine::SetBatchBlends with delays, host.py's three-tuples and render_aligned): two
channels share one source, one power amp's impulse response is the other's 37 samples later and negated.  The planner lines them up --
delays {37, 0}, signs {+1, -1} -- and the aligned blend carries the take's energy, where the blend of the same job as it stands nearly
cancels; the blend port written with those delays is the restatement (tests/blend_delay_ref.py) of the call's own chain rows."""
import numpy as np
import pytest

import blend_delay_ref as ref
import __graft_entry__ as entry
from helpers import synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
SR, NCH, BLOCKS, SHIFT = 48000, 2, 3, 37
NO = NCH + 3


@pytest.fixture(scope="module")
def host():
    entry.load_package()                                                 # build() has made both libraries
    from go_dsp_guitar_amd import host as h
    return h


def _engine(host):
    """two chains of one power amp each: the cabinet, and the same cabinet 37 samples later with its polarity turned -- both responses of one
    length and one energy, so that the filter compilation treats them alike"""
    base = synth_ir(2000, seed=5)
    irs = host.ImpulseResponses()
    irs.add("Near", SR, -20, np.concatenate([base, np.zeros(40)]))
    irs.add("Far", SR, -20, -np.concatenate([np.zeros(SHIFT), base, np.zeros(40 - SHIFT)]))
    eng = host.Engine(NCH, BLOCK)
    for c, name in enumerate(("Near", "Far")):
        ch = eng.create_chain(irs)
        ch.SetBypass(ch.AppendUnit(19), False)                            # the power amp alone: the chain is linear
        ch.SetDiscreteValue(0, "filter_1", name)
    sp = host.Spatializer(eng, NCH)
    sp.SetSampleRate(SR)
    for c in range(NCH):
        sp.SetAzimuth(c, -30.0 + 60.0 * c); sp.SetDistance(c, 1.0); sp.SetLevel(c, 0.9)
    eng.batch_set_sources([0, 0])                                         # one take through two rigs
    return eng, sp


def _inputs():
    enc = lambda x: np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)
    return [(enc(0.5 * synth_signal(0, BLOCKS * BLOCK - 300, SR)), "lpcm16", SR), None]


def test_render_aligned_lines_up_a_late_and_inverted_rig(host):
    inputs = _inputs()
    blend = [[(0, 0.5), (1, 0.5)]]
    eng, sp = _engine(host)
    unaligned = [o.view(np.float64).copy() for o in eng.batch_run(inputs, SR, "ieee64", window=2, blends=blend, report=True)]
    before = eng.last_report.copy()
    del sp
    eng.close()
    eng, sp = _engine(host)
    outs, delays, signs = eng.render_aligned(blend, 64, 0.5, inputs, SR, "ieee64", window=2, report=True)
    after = eng.last_report.copy()
    assert eng.last_error() == "" and len(outs) == NO + 1
    assert delays == [[SHIFT, 0]] and signs == [[1, -1]]
    # pass 1 measured channel 1 against channel 0: late by 37 samples, inverted, in every block
    rec = eng.aligned_records
    assert rec.shape == (NO, BLOCKS) and np.all(rec["lag"][1] == SHIFT) and np.all(rec["corr"][1] < 0) and not rec[0].view(np.uint8).any()
    rows = [o.view(np.float64) for o in outs]
    for c in range(NCH):                                                   # the chain files do not know about the blend
        assert np.array_equal(rows[c], unaligned[c]), c
    want = ref.blend(np.stack(rows[:NCH]), [(0, 0.5, SHIFT), (1, -0.5, 0)])
    assert ref.same_bits(rows[NO], want)
    # the aligned blend carries the take; the blend as it stood nearly cancels
    assert before.shape == after.shape == (NO + 1, BLOCKS)
    e_aligned, e_unaligned, e_chain = after["sum_sq"][NO].sum(), before["sum_sq"][NO].sum(), after["sum_sq"][0].sum()
    print("sum of squares: aligned %.6g, unaligned %.6g, channel 0 %.6g" % (e_aligned, e_unaligned, e_chain))
    assert e_aligned > e_unaligned and e_aligned > 0.9 * e_chain
    del sp
    eng.close()


def test_three_tuples_reach_the_library_and_refusals_name_the_term(host):
    eng, sp = _engine(host)
    assert eng._set_blends([[(0, 1.0, 5), (1, 1.0)]]) == 1
    for blends, what in (([[(0, 1.0, 4097)]], "blend 0, term 0: delay = 4097"), ([[(0, 1.0)], [(1, 1.0, 0), (0, 1.0, -1)]], "blend 1, term 1: delay = -1")):
        with pytest.raises(host.HostError, match=what):
            eng._set_blends(blends)
        assert host.lib().gdgh_engine_batch_blends(eng._h) == 1
    outs = eng.batch_run(_inputs(), SR, "ieee64", window=2, blends=[[(0, 1.0, 0), (0, -1.0, 1)]])
    assert eng.raw_context(0).batch_blend_max_delay() == 1
    rows = [o.view(np.float64) for o in outs]
    assert rows[0].any() and np.array_equal(rows[NO], np.concatenate([rows[0][:1], np.diff(rows[0])]))      # the known answer: the first difference
    del sp
    eng.close()
