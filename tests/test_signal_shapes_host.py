"""The yardstick of test_gpu_signal_shapes.py, checked before any kernel is held to it (CPU only): the oracle alone on the signal family of
tests/signal_shapes.py, every row of test_gpu_parity.UNIT_CASES, the three (rate, frames) pairs of signal_shapes.PAIRS.

Measured (60 rows x 13 signals x 3 pairs, 15 s):
  * every output is finite;
  * no (row, signal, rate) is ill-conditioned: the largest move under x * (1 + 2**-50) stays below 1e-10 * max(1, peak).  The issue that
    asked for this test expected the three `excess` rows in the table at a gain of 1000; they are not (signal_shapes.ILL_CONDITIONED);
  * the rows of CUT_INVARIANT give the same bits cut into the pair's frames and into 1024s on every signal, but for ONE row at one rate: the
    123 Hz square of the signal generator at 22050 Hz, one sample (signal_shapes.CUT_EXCEPTIONS).  The schedule of test_frame_lengths_host.py
    happened not to put a call boundary where it matters; calls of 1000 do.  The difference is pinned here, sample and size;
  * one non-finite input sample: the oracle is causal and contained for 37 of the 39 rows of CUT_INVARIANT; on the two auto-yoy rows the
    reference panics (signal_shapes.POISON_DROPPED), and the oracle, which has no bounds check, is not run there."""
import numpy as np
import pytest

from frame_lengths import oversampling_factor
from helpers import synth_signal
from signal_shapes import (CUT_EXCEPTIONS, ILL_CONDITIONED, NAMES, PAIRS, POISON_AT, POISON_DROPPED, impulse_at, key, oracle_row, row_channel,
                           signals)
from test_frame_lengths_host import CUT_INVARIANT
from test_gpu_fuzz import reference_panics
from test_gpu_parity import UNIT_CASES

SHAPERS = ("overdrive", "distortion", "excess", "fuzz")
FOLLOWERS = ("compressor", "auto_yoy", "auto_wah", "octaver")
HIGH_PASSES = ("tone_stack", "cabinet", "bandpass", "octaver", "auto_wah")
DELAY_RINGS = ("delay", "chorus", "flanger", "phaser", "auto_yoy")
# what each signal is aimed at: every row of these units must answer it with other bits than it answers plain `base` with
AIMED_AT = {
    "loud8": SHAPERS + ("auto_wah", "bandpass"),
    "loud1000": SHAPERS + ("auto_wah", "bandpass", "compressor"),
    "tiny": FOLLOWERS + HIGH_PASSES,
    "subnormal": FOLLOWERS + HIGH_PASSES,
    "silence": FOLLOWERS + HIGH_PASSES + SHAPERS + DELAY_RINGS,
    "burst_then_silence": FOLLOWERS + DELAY_RINGS,
    "silence_then_burst": FOLLOWERS + DELAY_RINGS,
    "impulse": DELAY_RINGS + HIGH_PASSES,
    "dc": HIGH_PASSES,
    "step": HIGH_PASSES,
    "square_full_scale": SHAPERS + ("compressor",),
    "nyquist": HIGH_PASSES + SHAPERS,
    "negative_zero_run": FOLLOWERS + ("delay",),
}


def even_cut(n):
    return [1024] * (n // 1024) + ([n % 1024] if n % 1024 else [])


@pytest.fixture(scope="module")
def measured(oracle):
    """Per pair: want[signal][k], want of plain base [k], the move under x (1 + 2**-50) [signal][k], and for the rows of CUT_INVARIANT the
    samples at which the cut into 1024s differs [signal][k].  Computed once for the tests below."""
    out = {}
    for sr, frames, calls in PAIRS:
        n = frames * calls
        cuts = [frames] * calls
        want = {name: [] for name in NAMES}
        moved = {name: [] for name in NAMES}
        cut_diff = {name: {} for name in NAMES}
        plain = []
        for k, (unit, params) in enumerate(UNIT_CASES):
            plain.append(oracle_row(oracle, unit, params, synth_signal(row_channel(k), n, sr), cuts, sr))
            for name, x in signals(row_channel(k), n, sr, frames).items():
                w = oracle_row(oracle, unit, params, x, cuts, sr)
                w2 = oracle_row(oracle, unit, params, x * (1.0 + 2.0 ** -50), cuts, sr)
                want[name].append(w)
                with np.errstate(invalid="ignore"):
                    moved[name].append(float(np.max(np.abs(w - w2))))
                if (unit, params) in CUT_INVARIANT:
                    cut_diff[name][k] = np.nonzero(w != oracle_row(oracle, unit, params, x, even_cut(n), sr))[0].tolist()
        out[sr] = dict(want=want, moved=moved, cut_diff=cut_diff, plain=plain)
    return out


def test_no_pair_of_the_three_is_one_on_which_the_reference_panics():
    for sr, frames, calls in PAIRS:
        for f, taps in ((2, 77), (4, 155)):
            assert not reference_panics(f * frames, taps), (frames, f)


def test_the_family():
    sr, frames, calls = PAIRS[1]
    n = frames * calls
    s = signals(3, n, sr, frames)
    base = synth_signal(3, n, sr)
    assert tuple(s) == NAMES and len(NAMES) == 13
    assert np.array_equal(s["loud8"], 8 * base) and np.array_equal(s["loud1000"], 1000 * base) and np.abs(s["loud8"]).max() > 4
    # a follower's first product, |x| (1 - exp(-20 / sr)), is below the smallest normal double for every sample, at every rate of PAIRS
    assert 0 < np.abs(s["subnormal"]).max() * (1.0 - np.exp(-20.0 / 22050)) < 2.2250738585072014e-308 and np.count_nonzero(s["subnormal"]) > 0.99 * n
    assert not s["silence"].any()
    assert np.array_equal(s["burst_then_silence"][:1500], base[:1500]) and not s["burst_then_silence"][1500:].any()
    assert not s["silence_then_burst"][:2500].any() and np.array_equal(s["silence_then_burst"][2500:], base[2500:])
    assert np.nonzero(s["impulse"])[0].tolist() == [impulse_at(frames)] == [1333] and s["impulse"][1333] == 1.0
    assert set(s["dc"]) == {0.5}
    assert set(s["step"][:1400]) == {-0.25} and set(s["step"][1400:]) == {0.75}
    assert set(s["square_full_scale"]) == {1.0, -1.0} and np.array_equal(s["square_full_scale"][:74], [1.0] * 37 + [-1.0] * 37)
    assert np.array_equal(s["square_full_scale"][74:148], s["square_full_scale"][:74])
    assert np.array_equal(s["nyquist"][:4], [0.9, -0.9, 0.9, -0.9])
    run = s["negative_zero_run"][1250:3250]
    assert not run.any() and np.signbit(run).all() and s["negative_zero_run"][1249] != 0 and s["negative_zero_run"][3250] != 0
    big = signals(3, 4 * 8192, 48000, 8192)
    assert np.nonzero(big["impulse"])[0].tolist() == [8192 + 2730] and not big["silence_then_burst"][:20480].any() and big["silence_then_burst"][20480] != 0


def test_the_oracle_is_finite_on_every_row_signal_and_pair(measured):
    for sr, frames, calls in PAIRS:
        for name in NAMES:
            assert len(measured[sr]["want"][name]) == len(UNIT_CASES) == 60
            for k, row in enumerate(UNIT_CASES):
                w = measured[sr]["want"][name][k]
                assert w.shape == (frames * calls,) and np.isfinite(w).all(), (sr, name, row)


def test_the_ill_conditioned_table_is_what_the_measurement_finds(measured):
    found = set()
    for sr, frames, calls in PAIRS:
        for name in NAMES:
            for k, (unit, params) in enumerate(UNIT_CASES):
                peak = float(np.max(np.abs(measured[sr]["want"][name][k])))
                if not measured[sr]["moved"][name][k] <= 1e-10 * max(1.0, peak):
                    found.add(key(unit, params) + (name, sr))
    assert found == set(ILL_CONDITIONED), (sorted(found - set(ILL_CONDITIONED)), sorted(set(ILL_CONDITIONED) - found))
    for sr, frames, calls in PAIRS:
        assert sum(1 for t in ILL_CONDITIONED if t[3] == sr) <= 3, sr
    assert not [t for t in ILL_CONDITIONED if t[2] in ("silence", "impulse", "dc", "square_full_scale", "loud8")]
    assert all(isinstance(reason, str) and ".go:" in reason for reason in ILL_CONDITIONED.values())


def test_cut_invariant_rows_do_not_depend_on_the_cut_on_any_signal(measured):
    """frames of the pair against 1024s, bit for bit; the exceptions are pinned to the sample"""
    seen = set()
    for sr, frames, calls in PAIRS:
        for name in NAMES:
            for k, (unit, params) in enumerate(UNIT_CASES):
                if (unit, params) not in CUT_INVARIANT:
                    continue
                differs = measured[sr]["cut_diff"][name][k]
                exception = CUT_EXCEPTIONS.get(key(unit, params) + (sr,))
                if exception:
                    assert differs == exception[0], (sr, name, unit, params, differs)
                    seen.add(key(unit, params) + (sr,))
                else:
                    assert differs == [], "%s %s at %d Hz on %s: the oracle's output depends on the cut at samples %s" % (
                        unit, params, sr, name, differs[:8])
    assert seen == set(CUT_EXCEPTIONS) and len(CUT_EXCEPTIONS) == 1


def test_every_signal_reaches_what_it_is_aimed_at(measured):
    assert set(AIMED_AT) == set(NAMES)
    for sr, frames, calls in PAIRS:
        m = measured[sr]
        for name in NAMES:
            hit = 0
            for k, (unit, params) in enumerate(UNIT_CASES):
                if unit in AIMED_AT[name]:
                    assert not np.array_equal(m["want"][name][k], m["plain"][k]), (sr, name, unit, params)
                    hit += 1
            assert hit >= 5, (name, hit)
        for k, (unit, params) in enumerate(UNIT_CASES):
            w = m["want"]["silence"][k]
            if unit == "signal_generator":
                assert w.any(), (sr, params)                         # the one unit with a source of its own
            else:
                assert not w.any(), (sr, unit, params)               # exact zeros (of either sign) out of exact zeros
            # above full scale the shapers leave the range the smooth signal keeps them in, and the impulse comes out of a delay ring late
            if unit in SHAPERS:
                assert not np.array_equal(m["want"]["loud8"][k], m["want"]["loud1000"][k]), (sr, unit, params)
            if unit == "delay":
                w = m["want"]["impulse"][k]
                assert w[impulse_at(frames)] != 0 and not w[:impulse_at(frames)].any(), (sr, params)
                if params == [3, -10, 0]:                            # 3 ms: its echo lies inside every one of these streams
                    echo = impulse_at(frames) + int(0.003 * sr + 0.5)
                    assert np.nonzero(w)[0].tolist() == [impulse_at(frames), echo], (sr, np.nonzero(w)[0].tolist())
            # the silent stretches: a causal time-domain row is silent until the burst comes
            if (unit, params) in CUT_INVARIANT and unit != "signal_generator":
                assert not m["want"]["silence_then_burst"][k][:2 * frames + frames // 2].any(), (sr, unit, params)
                assert np.array_equal(m["want"]["burst_then_silence"][k][:frames + frames // 2], m["plain"][k][:frames + frames // 2]), (sr, unit, params)


# ---- part (c): one non-finite sample -----------------------------------------------------------------------------------------------------
def poison_rows():
    """the rows of CUT_INVARIANT without oversampling that the reference can run with a non-finite sample, as indices into UNIT_CASES"""
    return [k for k, (unit, params) in enumerate(UNIT_CASES)
            if (unit, params) in CUT_INVARIANT and oversampling_factor(unit, params) == 1 and key(unit, params) not in POISON_DROPPED]


def test_rows_dropped_from_the_poison_test_are_named_and_few():
    assert len(POISON_DROPPED) <= 4
    rows = [key(*row) for row in CUT_INVARIANT]
    for dropped, reason in POISON_DROPPED.items():
        assert dropped in rows and dropped[0] == "auto_yoy" and "autoyoy.go:" in reason
    assert all(oversampling_factor(*row) == 1 for row in CUT_INVARIANT)
    assert len(poison_rows()) == len(CUT_INVARIANT) - len(POISON_DROPPED) == 37


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_the_oracle_keeps_a_non_finite_sample_behind_itself(oracle, poison):
    """Every output sample before the poisoned one has the bits of the run whose sample is 0.0 instead: the reference is causal for these rows.
    (The two auto-yoy rows are not run: the reference panics there, and the oracle would index out of its buffer.)"""
    sr, frames, calls = PAIRS[1]
    n, at = frames * calls, frames + POISON_AT
    for k in poison_rows():
        unit, params = UNIT_CASES[k]
        x = synth_signal(row_channel(k), n, sr)
        x[at] = 0.0
        clean = oracle_row(oracle, unit, params, x, [frames] * calls, sr)
        x[at] = poison
        got = oracle_row(oracle, unit, params, x, [frames] * calls, sr)
        assert np.isfinite(clean).all(), (unit, params)
        assert np.array_equal(got[:at], clean[:at]), (unit, params)
        assert got.shape == clean.shape
