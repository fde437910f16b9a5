"""A short FIR per blend term through the C++ twin (Engine::SetBatchBlends with taps, host.py's four-tuples and
render_aligned(fraction_steps=4)): two channels share one source, noise band-limited below 0.4 of the sample rate; the power amps' impulse
responses are windowed sincs centred 37.5 samples apart.  Whole samples leave half a sample between the rigs; the pass between the planner
and the render finds it -- the planned total offset is 37.5 samples -- and the aligned blend's sum of squares lies above that of the
integer-aligned blend of the same job.  fraction_steps=0 returns what it returned before.  The numpy planner below is run first, without a
device: it is how the input's seed was chosen (DESIGN.md 4.12f carries the seed and the two energies)."""
import numpy as np
import pytest

import blend_delay_ref as delay_ref
import blend_filter_ref as ref
import __graft_entry__ as entry

BLOCK = 8192
SR, NCH, BLOCKS = 48000, 2, 3
NO = NCH + 3
SEED, Q, T = 1, 4, 32
SAMPLES = BLOCKS * BLOCK - 300
CENTRES = (64.0, 101.5)                                                      # 37.5 samples apart


def sinc_ir(centre, length=160, half=40):
    """sinc(n - centre) under a raised-cosine window of +-half samples around the centre: at 64.0 the unit impulse, at 101.5 half a sample between two"""
    u = np.arange(length, dtype=np.float64) - centre
    return np.sinc(u) * np.where(np.abs(u) <= half, 0.5 + 0.5 * np.cos(np.pi * u / half), 0.0)


def take(seed=SEED):
    """white noise with everything at and above 0.4 of the sample rate removed, as the 16-bit file the job reads"""
    x = np.random.default_rng(seed).standard_normal(SAMPLES)
    X = np.fft.rfft(x)
    X[np.arange(X.size) / float(SAMPLES) >= 0.4] = 0.0
    x = np.fft.irfft(X, SAMPLES)
    return np.round(0.25 * x / np.max(np.abs(x)) * 32767.0) / 32767.0


def numpy_plan(seed=SEED):
    """the plan without the library: the whole-sample lag of the far rig from the cross-correlation of the first block, then the candidate of
    2Q - 1 around it with the largest tx / sqrt(xx) against the near rig delayed by the common latency -> (total offset, aligned energy, integer energy)"""
    x = take(seed)
    rows = np.stack([np.convolve(x, sinc_ir(c))[:SAMPLES] for c in CENTRES])
    corr = [abs(np.dot(rows[0][:BLOCK - 64], rows[1][lag:lag + BLOCK - 64])) for lag in range(65)]
    lag = int(np.argmax(corr))
    root = ref.blend(rows, [(0, 1.0, lag + T // 2)])
    scores = []
    for step in range(-(Q - 1), Q):
        num = Q + step                                                       # the far rig's whole-sample delay is 0: n + f = 1 + step / Q
        cand = ref.blend(rows, [(1, 1.0, num // Q, ref.fraction_taps(T, (num % Q) / float(Q)))])
        scores.append(np.dot(root, cand) / np.sqrt(np.dot(cand, cand)))
    step = int(np.argmax(scores)) - (Q - 1)
    num = Q + step
    aligned = ref.blend(rows, [(0, 0.5, lag + T // 2), (1, 0.5, num // Q, ref.fraction_taps(T, (num % Q) / float(Q)))])
    integer = ref.blend(rows, [(0, 0.5, lag), (1, 0.5, 0)])
    return lag - step / float(Q), float(np.sum(aligned ** 2)), float(np.sum(integer ** 2))


def test_the_numpy_planner_alone_gives_37_5_for_the_seed():
    total, aligned, integer = numpy_plan()
    print("seed %d: total offset %.2f, aligned %.6g, integer-aligned %.6g" % (SEED, total, aligned, integer))
    assert total == 37.5 and aligned > integer


@pytest.fixture(scope="module")
def host():
    entry.load_package()                                                 # build() has made both libraries
    from go_dsp_guitar_amd import host as h
    return h


def _engine(host):
    irs = host.ImpulseResponses()
    for name, centre in zip(("Near", "Far"), CENTRES):
        irs.add(name, SR, -20, sinc_ir(centre))
    eng = host.Engine(NCH, BLOCK)
    for name in ("Near", "Far"):
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
def test_render_aligned_finds_the_half_sample_between_two_rigs(host):
    inputs = _inputs()
    blend = [[(0, 0.5), (1, 0.5)]]
    eng, sp = _engine(host)
    whole = eng.render_aligned(blend, 64, 0.5, inputs, SR, "ieee64", window=2, report=True, fraction_steps=0)
    integer_report = eng.last_report.copy()
    assert len(whole) == 3                                                # fraction_steps=0: (outs, delays, signs), as before
    outs0, delays0, signs0 = whole
    rows0 = [o.view(np.float64).copy() for o in outs0]
    assert signs0 == [[1, 1]] and delays0 in ([[37, 0]], [[38, 0]])
    assert delay_ref.same_bits(rows0[NO], delay_ref.blend(np.stack(rows0[:NCH]), [(0, 0.5, delays0[0][0]), (1, 0.5, 0)]))      # today's values
    del sp
    eng.close()
    eng, sp = _engine(host)
    outs, delays, signs, fractions = eng.render_aligned(blend, 64, 0.5, inputs, SR, "ieee64", window=2, report=True, fraction_steps=Q, fraction_taps=T)
    report = eng.last_report.copy()
    assert eng.last_error() == "" and len(outs) == NO + 1 and delays == delays0 and signs == signs0
    total = (delays[0][0] + fractions[0][0]) - (delays[0][1] + fractions[0][1])
    assert total == 37.5 and fractions[0][0] == 0.0, (delays, fractions)
    assert eng.fraction_records.shape == (1, BLOCKS) and np.all(eng.fraction_records["terms"] == 2 * Q - 1)
    rows = [o.view(np.float64) for o in outs]
    for c in range(NCH):                                                   # the chain files do not know about the blend
        assert np.array_equal(rows[c], rows0[c]), c
    # the blend port is the restatement of the call's own chain rows: every term T/2 samples later than the whole-sample plan
    num = (delays[0][1] + 1) * Q + int(round(fractions[0][1] * Q))
    got_taps = entry.load_package().blend_fraction_taps(T, (num % Q) / float(Q))      # the library's own taps: the sum over them is exact
    assert np.max(np.abs(got_taps - ref.fraction_taps(T, (num % Q) / float(Q)))) <= (2 * T + 16) * 2.0 ** -52
    assert ref.same_bits(rows[NO], ref.blend(np.stack(rows[:NCH]), [(0, 0.5, delays[0][0] + T // 2), (1, 0.5, num // Q, got_taps)]))
    assert eng.raw_context(0).batch_blend_max_reach() == max(delays[0][0] + T // 2, num // Q + T - 1)
    e_aligned, e_integer = report["sum_sq"][NO].sum(), integer_report["sum_sq"][NO].sum()
    print("plan: delays %s, fractions %s" % (delays, fractions))
    print("sum of squares: aligned to a quarter sample %.6g, integer-aligned %.6g, channel 0 %.6g" % (e_aligned, e_integer, report["sum_sq"][0].sum()))
    assert e_aligned > e_integer
    del sp
    eng.close()


@pytest.mark.gpu
def test_four_tuples_reach_the_library_and_refusals_name_blend_and_term(host):
    eng, sp = _engine(host)
    assert eng._set_blends([[(0, 1.0, 5, [1.0, -1.0]), (1, 1.0)]]) == 1
    for blends, what in (([[(0, 1.0, 0, np.ones(65))]], "blend 0, term 0 has 65 taps"), ([[(0, 1.0)], [(1, 1.0, 0), (0, 1.0, 0, [1.0, np.nan])]], "blend 1, term 1: tap 1"),
                         ([[(0, 1.0, 4095, [1.0, 1.0, 1.0])]], "blend 0, term 0: a delay of 4095 samples and 3 taps")):
        with pytest.raises(host.HostError, match=what):
            eng._set_blends(blends)
        assert host.lib().gdgh_engine_batch_blends(eng._h) == 1
    outs = eng.batch_run(_inputs(), SR, "ieee64", window=2, blends=[[(0, 1.0, 0, [1.0, -1.0])]])
    assert eng.raw_context(0).batch_blend_max_reach() == 1 and eng.raw_context(0).batch_blend_max_delay() == 0
    rows = [o.view(np.float64) for o in outs]
    assert rows[0].any() and np.array_equal(rows[NO], np.concatenate([rows[0][:1], np.diff(rows[0])]))      # the known answer: the first difference
    # a plan that would reach past 4096 samples names the blend
    with pytest.raises(host.HostError, match="render_aligned: blend 0"):
        eng._render_fractions(entry.load_package(), [[(0, 0.5), (1, 0.5)]], [[4090, 0]], [[1, 1]], [-1, 0, -1, -1, -1], Q, T, None, SR, _inputs(), SR, "ieee64", 2, {})
    del sp
    eng.close()
