"""The tap fit end to end through the C++ twin (Engine::SetBatchTapFits, host.py's tapfits= and render_tap_fitted): white noise shared by two
channels, channel 0 through a power amp with a random 12-tap response, channel 1 through a unit impulse; the 16 taps on channel 1 that come
closest to channel 0 are the 12 and four zeros.  The reference is numpy.linalg.lstsq on the shifted rows of the call's own float64 files.
The tolerance is FACTOR * U * 2^-52 * cond(A), cond(A) from the reference's singular values; FACTOR comes from the numpy restatement of
the planner (tests/tapfit_ref.py) against lstsq on rows made on the CPU, seeds 1 to 8, times a margin of 4 for the device's other order of
summation -- the first test below measures it again, without a device (DESIGN.md 4.12g carries the figures)."""
import numpy as np
import pytest

import blend_filter_ref as filter_ref
import tapfit_ref as ref
import __graft_entry__ as entry

BLOCK = 8192
SR, NCH, BLOCKS = 48000, 2, 3
NO = NCH + 3
SAMPLES = BLOCKS * BLOCK - 300
TAPS, IR_TAPS = 16, 12
EPS = 2.0 ** -52
FACTOR = 3.4                                                                 # 4 x 0.844, the worst of seeds 1 .. 8 below


def take(seed=1):
    """white noise as the 16-bit file the job reads"""
    x = np.random.default_rng(seed).standard_normal(SAMPLES)
    return np.round(0.25 * x / 4.0 * 32767.0).clip(-32767, 32767) / 32767.0


def amp_ir(seed=1):
    return np.random.default_rng(100 + seed).uniform(-1.0, 1.0, IR_TAPS)


def test_the_factor_is_four_times_the_worst_of_eight_seeds_on_cpu_made_rows():
    worst, worst_res = 0.0, 0.0
    for seed in range(1, 9):
        x = take(seed)
        rows = np.stack([np.convolve(x, amp_ir(seed))[:SAMPLES], x])
        fits = [(0, [1], TAPS)]
        recs = []
        for b in range(BLOCKS):
            v = ref.shifted_rows(rows, 0, [1], TAPS, b * BLOCK, min(BLOCK, SAMPLES - b * BLOCK))
            recs.append(ref.packed(v @ v.T))
        (h, res), = ref.plan(np.stack(recs), fits)
        h_ref, res_ref, cond = ref.lstsq_taps(rows, 0, [1], TAPS, BLOCK)
        unit = TAPS * EPS * cond
        worst = max(worst, np.max(np.abs(h - h_ref)) / np.max(np.abs(h_ref)) / unit)
        worst_res = max(worst_res, abs(res - res_ref) / unit)
    print("worst max|h - h_ref| / max|h_ref| over seeds 1 .. 8: %.3f x U 2^-52 cond(A); the residual's: %.3f" % (worst, worst_res))
    assert 4.0 * worst <= FACTOR and 4.0 * worst_res <= FACTOR, (worst, worst_res)
    assert FACTOR <= 8.0 * worst, "the factor is the measured one, not a wider one"


@pytest.fixture(scope="module")
def host():
    entry.load_package()                                                 # build() has made both libraries
    from go_dsp_guitar_amd import host as h
    return h


def _engine(host):
    irs = host.ImpulseResponses()
    unit = np.zeros(IR_TAPS)
    unit[0] = 1.0
    irs.add("Amp", SR, -20, amp_ir())
    irs.add("Wire", SR, -20, unit)
    eng = host.Engine(NCH, BLOCK)
    for name in ("Amp", "Wire"):
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
    return [(np.ascontiguousarray(np.round(take() * 32767.0).astype("<i2")).view(np.uint8), "lpcm16", SR), None]


@pytest.mark.gpu
def test_render_tap_fitted_finds_the_amp_s_response(host):
    eng, sp = _engine(host)
    outs, h, residual = eng.render_tap_fitted(0, [1], TAPS, _inputs(), SR, "ieee64", center=0, window=2)
    assert eng.last_error() == "" and len(outs) == NO + 1 and h.shape == (1, TAPS)
    assert eng.tap_fitted_records.shape == (BLOCKS, ref.fit_doubles(1, TAPS))
    rows = np.stack([o.view(np.float64) for o in outs])
    assert rows.shape == (NO + 1, BLOCKS * BLOCK) and all(r.any() for r in rows[:NCH])
    h_ref, res_ref, cond = ref.lstsq_taps(rows[:NCH], 0, [1], TAPS, BLOCK)
    tol = FACTOR * TAPS * EPS * cond
    err = np.max(np.abs(h - h_ref)) / np.max(np.abs(h_ref))
    print("cond(A) %.4f, max|h - h_ref| / max|h_ref| %.3g (tolerance %.3g), residual %.3g against %.3g" % (cond, err, tol, residual, res_ref))
    assert err <= tol, (err, tol)
    assert abs(residual - res_ref) <= tol, (residual, res_ref, tol)
    assert np.max(np.abs(h[0, IR_TAPS:])) <= tol * np.max(np.abs(h_ref)), "the amp has 12 taps: the last four are zero within the tolerance"
    # the blend port rendered with the planned taps is the restatement applied to the call's own files
    assert filter_ref.same_bits(rows[NO], filter_ref.blend(rows[:NCH], [(1, 1.0, 0, h[0])]))
    del sp
    eng.close()


@pytest.mark.gpu
def test_tapfits_reach_the_library_and_refusals_name_the_term(host):
    pkg = entry.load_package()
    eng, sp = _engine(host)
    assert eng._set_tapfits([(0, [1], 16), (1, [0, 0], 3)]) == 2
    for fits, what in (([(0, [1], 65)], "fit 0 has 65 taps per term"), ([(0, [1, 0, 1], 64)], "fit 0 has 3 terms x 64 taps = 192 unknowns"), ([(0, [1], 4), (0, [-1], 4)], "fit 1, term 0 names port -1")):
        with pytest.raises(host.HostError, match=what):
            eng._set_tapfits(fits)
        assert host.lib().gdgh_engine_batch_tapfits(eng._h) == 2
    eng.batch_run(_inputs(), SR, "ieee64", window=2, tapfits=[(0, [1], 4)], skip_outputs=True)
    assert eng.last_tapfit.shape == (BLOCKS, ref.fit_doubles(1, 4)) and eng.last_tapfit.any()
    parts = list(eng.batch_stream(_inputs(), SR, "ieee64", 2, window=2, tapfits=[(0, [1], 4)]))
    assert len(parts) == 2 and eng.last_tapfit.shape == (BLOCKS, ref.fit_doubles(1, 4))
    with pytest.raises(host.HostError, match="term 0 reaches 4090 \\+ 16 - 1 = 4105 samples back"):
        eng.render_tap_fitted(0, [1], TAPS, _inputs(), SR, "ieee64", delays=[4090], center=0)
    with pytest.raises(host.HostError, match="only a chain output"):
        eng.render_tap_fitted(NCH, [1], TAPS, _inputs(), SR, "ieee64")
    # a delayed, inverted term and a centred target: the records name blend ports, and the blend lags the target by `center`
    outs, h, residual = eng.render_tap_fitted(0, [1], TAPS, _inputs(), SR, "ieee64", delays=[3], signs=[-1], center=5, window=2)
    rows = np.stack([o.view(np.float64) for o in outs])
    assert filter_ref.same_bits(rows[NO], filter_ref.blend(rows[:NCH], [(1, -1.0, 3, h[0])]))
    measured = np.stack([filter_ref.blend(rows[:NCH], [(0, 1.0, 5)]), filter_ref.blend(rows[:NCH], [(1, -1.0, 3)])])      # what pass 1 measured
    h_ref, res_ref, cond = ref.lstsq_taps(measured, 0, [1], TAPS, BLOCK)
    tol = FACTOR * TAPS * EPS * cond
    assert np.max(np.abs(h - h_ref)) / np.max(np.abs(h_ref)) <= tol and abs(residual - res_ref) <= tol, (h, h_ref, residual, res_ref)
    quiet = np.concatenate([h[0, :2], h[0, 2 + IR_TAPS:]])
    assert np.max(np.abs(quiet)) <= tol * np.max(np.abs(h_ref)) and h[0, 2:2 + IR_TAPS].all(), "the response begins 5 - 3 samples later"
    assert pkg.TAPFIT_MAX_TERMS == 4
    del sp
    eng.close()
