"""The yardstick of test_gpu_frame_lengths.py, checked before any kernel is held to it (CPU only).

1. The schedule (tests/frame_lengths.py): its totals, and every ring capacity with both neighbours.
2. The oracle alone: every row of test_gpu_parity.UNIT_CASES at the three rates, the stream cut by schedule(sr) against the same stream cut
   into 1024s.  The reference's sample loops are sequential, so most units cannot depend on the cut; where the oracle did at a short frame, the
   oracle would be what is wrong there, not a kernel.

Measured (60 rows x 3 rates, 4 s):
  * bit-identical, 39 rows (CUT_INVARIANT): every compressor, tone stack, cabinet, delay, tremolo, reverb, auto-yoy, auto-wah, band pass,
    octaver and noise gate row (30), the shapers and fuzzes without oversampling (7), signal generator types 2 and 4;
  * within 4e-13, 4 rows (CUT_ROUNDS): both ring modulators and signal generator types 0 and 1 -- the phase is carried as
    fmod(phase + N * increment), rounded once per call (effects/ringmodulator.go:42-44, effects/signalgenerator.go:60-61, :86-87);
  * the cut matters by design of the reference, 17 rows: the ten 2x / 4x oversampled shapers and fuzzes, which resample each block on its own by
    FFT (effects/overdrive.go:135-139, effects/fuzz.go:165-169); the six chorus, flanger and phaser rows, whose LFO phase is advanced by the
    buffer's duration at the end of the call while the samples inside count time from the buffer's start (effects/chorus.go:59-61, :116-118,
    effects/flanger.go:60-62, :103-104, effects/phaser.go:66-68, :109-110); and the sawtooth [100, 0, 3, 5000, 50, 0], whose 5 kHz period lands
    on its phase jump at 48 and 192 kHz (effects/signalgenerator.go:112-127).
The issue that asked for this test counted 44 / 4 / 12: it took the oversampled rows for nine and chorus, flanger and phaser for one row each.
The classes are the ones it describes; by row they are 39 / 4 / 17, and every row of UNIT_CASES is in exactly one (checked below)."""
import numpy as np
import pytest

from frame_lengths import MAX_FRAMES, RATES, decimator_pair, oversampling_factor, ring_capacities, schedule
from helpers import synth_signal
from test_gpu_fuzz import reference_panics
from test_gpu_parity import UNIT_CASES

TOTALS = {48000: (31, 47384), 22050: (31, 42326), 192000: (28, 46664)}          # rate: (calls, samples)

CUT_INVARIANT = [
    ("compressor", None), ("compressor", [0, 30, -20]), ("compressor", [1, 12, -6]),
    ("overdrive", None), ("overdrive", [10, 20, 70, -3, 0, 0]),
    ("distortion", [0, 20, -3, 0]),
    ("excess", [20, -3, 0]),
    ("tone_stack", None), ("tone_stack", [-10, 0, -3, -20]),
    ("cabinet", None),
    ("delay", None), ("delay", [3, -10, 0]), ("delay", [1000, 0, 0]),
    ("tremolo", None), ("tremolo", [10, 0, -60]), ("tremolo", [100, 100, -3]),
    ("signal_generator", [100, 0, 2, 123, 50, 0]), ("signal_generator", [30, 0, 4, 440, 100, -10]),
    ("reverb", None), ("reverb", [100]), ("reverb", [0]),
    ("fuzz", None), ("fuzz", [0, -30, 10, 20, 60, -3, 0]), ("fuzz", [1, 100, 0, 30, 100, 0, 0]),
    ("auto_yoy", None), ("auto_yoy", [0, -10, -50, 40]),
    ("auto_wah", None), ("auto_wah", [0, -5, -45, 200, 9000]),
    ("bandpass", None), ("bandpass", [3, 5000, 100]), ("bandpass", [1, 40, 18000]),
    ("octaver", None), ("octaver", [0, -6, -12, -3, 0, -6, -30]), ("octaver", [1, -60, 0, -60, -3, -3, 0]),
    ("noise_gate", None), ("noise_gate", [-10, -14, 5]), ("noise_gate", [-30, -20, 50]), ("noise_gate", [-6, -40, 0]),
    ("noise_gate", [-3, -8, 1]),
]
CUT_ROUNDS = [("ring_modulator", None), ("ring_modulator", [7]), ("signal_generator", None), ("signal_generator", [50, -6, 1, 1000, 80, -3])]
CUT_ROUNDS_TOL = 1e-12
CUT_MATTERS = [
    ("overdrive", [0, 20, 100, 0, 1, 1]), ("overdrive", [0, 20, 100, 0, 1, 2]), ("overdrive", [5, 10, 50, -6, 0, 2]),
    ("distortion", [0, 20, -3, 1]), ("distortion", [10, 10, 0, 2]), ("excess", [30, 0, 1]), ("excess", [12, -6, 2]),
    ("fuzz", [1, 50, 0, 20, 100, 0, 1]), ("fuzz", [0, 30, 10, 10, 70, -6, 2]), ("fuzz", [1, -50, 0, 30, 100, 0, 2]),
    ("chorus", None), ("chorus", [35, 77]), ("flanger", None), ("flanger", [40, 100]), ("phaser", None), ("phaser", [70, 33, -60]),
    ("signal_generator", [100, 0, 3, 5000, 50, 0]),
]


def test_schedule_totals():
    assert set(TOTALS) == set(RATES)
    for sr, (calls, samples) in TOTALS.items():
        s = schedule(sr)
        assert (len(s), sum(s)) == (calls, samples), (sr, len(s), sum(s))
        assert all(1 <= n <= MAX_FRAMES for n in s)


def test_every_ring_capacity_has_both_neighbours():
    assert ring_capacities(48000) == [96, 144, 480, 2400]
    assert ring_capacities(22050) == [44, 66, 221, 1103]            # 220.5 + 0.5 and 1102.5 + 0.5 round up
    assert ring_capacities(192000) == [384, 576, 1920, 9600]
    for sr in RATES:
        s = schedule(sr)
        for cap in ring_capacities(sr):
            if cap <= MAX_FRAMES - 1:
                at = [i for i in range(len(s) - 2) if s[i:i + 3] == [cap - 1, cap, cap + 1]]
                assert at, (sr, cap)
            else:
                assert cap not in s and cap > MAX_FRAMES        # the chorus ring at 192 kHz: longer than any frame


def test_the_three_lists_are_a_partition_of_the_unit_cases():
    listed = CUT_INVARIANT + CUT_ROUNDS + CUT_MATTERS
    assert len(listed) == len(UNIT_CASES) == 60
    assert (len(CUT_INVARIANT), len(CUT_ROUNDS), len(CUT_MATTERS)) == (39, 4, 17)
    for row in UNIT_CASES:
        assert listed.count(row) == UNIT_CASES.count(row) == 1, row


# lengths of the schedule at which the reference panics inside the decimator of a 2x or 4x oversampled unit (the same for both factors: the
# frame and the block, nextpow2 of 77 and of 155 taps, both double): filter/filter.go:370-382, :443-453 through oversampling.go:149-150
NO_REFERENCE = {22050: [1025, 2049, 3000, 4097, 1102, 1103, 1104],
                48000: [1025, 2049, 3000, 4097, 143, 144, 145, 2399, 2400, 2401],
                192000: [1025, 2049, 3000, 4097, 383, 384, 385, 575, 576, 577, 1919, 1920, 1921]}


def test_calls_on_which_the_reference_panics_in_a_decimator():
    """What test_gpu_frame_lengths.py may not hold to the oracle, worked out from the Go text alone: the oversampled rows and these lengths."""
    oversampled = [row for row in UNIT_CASES if oversampling_factor(*row) > 1]
    assert len(oversampled) == 10 and all(row in CUT_MATTERS for row in oversampled)
    assert decimator_pair("overdrive", [0, 20, 100, 0, 1, 1], 1025) == (2050, 77)
    assert decimator_pair("fuzz", [0, 30, 10, 10, 70, -6, 2], 3000) == (12000, 155)
    assert decimator_pair("overdrive", None, 1025) is None and decimator_pair("chorus", [35, 77], 1025) is None
    for sr in RATES:
        for row in oversampled:
            assert [n for n in schedule(sr) if reference_panics(*decimator_pair(row[0], row[1], n))] == NO_REFERENCE[sr], (sr, row)
    for n in (1, 2, 3, 7, 63, 64, 65, 1023, 2047, 8191, 8192):          # the short, the ragged-by-one-less and the full frames all have a reference
        assert not reference_panics(2 * n, 77) and not reference_panics(4 * n, 155), n


def _stream(oracle, unit, params, x, cuts, sr):
    ch = oracle.Chain()
    ch.append_unit(unit, params=params)
    out, pos = [], 0
    for n in cuts:
        out.append(ch.process(x[pos:pos + n], sr))
        pos += n
    assert pos == x.size
    return np.concatenate(out)


@pytest.fixture(scope="module")
def cut_difference(oracle):
    """max |schedule cut - 1024 cut| per (row index, rate), computed once for the tests below"""
    diff = {}
    for k, (unit, params) in enumerate(UNIT_CASES):
        for sr in RATES:
            s = schedule(sr)
            total = sum(s)
            x = synth_signal(7 * k + 3, total, sr)
            even = [1024] * (total // 1024) + ([total % 1024] if total % 1024 else [])
            a, b = _stream(oracle, unit, params, x, s, sr), _stream(oracle, unit, params, x, even, sr)
            assert np.isfinite(a).all() and np.isfinite(b).all(), (unit, params, sr)
            diff[k, sr] = float(np.max(np.abs(a - b)))
    return diff


def test_oracle_rows_that_cannot_depend_on_the_cut_do_not(cut_difference):
    for k, row in enumerate(UNIT_CASES):
        if row in CUT_INVARIANT:
            for sr in RATES:
                assert cut_difference[k, sr] == 0.0, "%s at %d Hz: the oracle's output depends on the cut, max %.3e" % (row, sr, cut_difference[k, sr])


def test_oracle_rows_whose_phase_rounds_per_call_stay_within_rounding(cut_difference):
    for k, row in enumerate(UNIT_CASES):
        if row in CUT_ROUNDS:
            for sr in RATES:
                assert cut_difference[k, sr] <= CUT_ROUNDS_TOL, "%s at %d Hz: max %.3e" % (row, sr, cut_difference[k, sr])


def test_oracle_rows_listed_as_cut_dependent_are(cut_difference):
    """Keeps the third list honest: a row in it that stopped depending on the cut belongs in the first."""
    for k, row in enumerate(UNIT_CASES):
        if row in CUT_MATTERS:
            assert max(cut_difference[k, sr] for sr in RATES) > 1e-6, row
