"""The CPU side of the filtered blend outputs (gdg_batch_set_blends_filtered, gdg_blend_fraction_taps, gdg_blend_fractions_from_fit):
csrc/blend.h -- the table packed without taps is the delayed table byte for byte, every refusal of the taps leaves the list in force as it
was and names blend and term, the filtered sum on the host against the known answer of include/gdg.h, the taps of a fractional delay and
the planner on hand-made fit records -- compiled without HIP into a stand-alone program under AddressSanitizer and UBSan, run directly;
then the restatement itself (tests/blend_filter_ref.py), and the two planners through the library's own entry points against it.  What the
kernel writes is tests/test_gpu_blend_filter.py's business."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import blend_filter_ref as ref

ROOT = entry.ROOT


@pytest.fixture(scope="module")
def filter_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blend_filter") / "blend_filter_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "go-dsp-guitar_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "blend_filter_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_the_table_the_refusals_the_known_answer_and_the_planners_under_the_sanitizers(filter_check):
    r = subprocess.run([filter_check], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr


def test_the_restatement_gives_the_first_difference_and_the_delayed_sum():
    """a self-check of the reference alone (tests/blend_filter_ref.py against numpy and blend_delay_ref): it calls nothing of the library and
    says nothing about the feature -- it keeps the yardstick of the other tests honest"""
    x = np.array([[0.5, -0.25, 3.0, 3.0, -0.0, 1e-300]])
    got = ref.blend(x, [(0, 1.0, 0, [1.0, -1.0])])
    assert np.array_equal(got, np.concatenate([x[0, :1], np.diff(x[0])])) and got[0] == x[0, 0] - 0.0
    assert ref.same_bits(got, ref.delay_ref.blend(x, [(0, 1.0, 0), (0, -1.0, 1)]))
    hist = np.full((1, ref.MAX_DELAY), 7.0)
    hist[0, -1], hist[0, 0] = 2.0, -4.0
    assert ref.blend(x, [(0, 1.0, 0, [1.0, -1.0])], hist)[0] == -1.5
    assert np.array_equal(ref.blend(x, [(0, 1.0, ref.MAX_DELAY - 1, [1.0, -1.0])], hist)[:2], [11.0, 0.0])
    # no taps: the delayed restatement; one tap: a second weight, rounded on its own
    terms = [(0, 0.5, 1), (0, 2.0, 3)]
    assert ref.same_bits(ref.blend(x, [t + ([],) for t in terms], hist), ref.delay_ref.blend(x, terms, hist))
    assert ref.same_bits(ref.blend(x, [(0, 0.1, 0, [0.3])]), np.float64(0.1) * (np.float64(0.3) * x[0]))
    assert ref.reach((0, 1.0)) == 0 and ref.reach((0, 1.0, 5)) == 5 and ref.reach((0, 1.0, 5, [1.0])) == 5 and ref.reach((0, 1.0, 5, np.ones(64))) == 68


def test_the_library_s_fraction_taps_are_the_restatement(pkg):
    """(2T + 16) * 2^-52 absolute: two transcendental calls of a few ulp per tap and a normalising sum of T taps give a relative error of
    order T ulp, and every |h| <= 1 up to that same relative error"""
    for T in (2, 4, 24, 32, 62, 64):
        bound = (2 * T + 16) * 2.0 ** -52
        for f in (0.0, 0.125, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.999, 1e-9):
            got, want = pkg.blend_fraction_taps(T, f), ref.fraction_taps(T, f)
            assert got.shape == (T,) and np.max(np.abs(got - want)) <= bound, (T, f, np.max(np.abs(got - want)), bound)
            assert abs(float(np.sum(got)) - 1.0) <= bound and np.max(np.abs(got)) <= 1.0 + bound
        impulse = pkg.blend_fraction_taps(T, 0.0)
        assert np.array_equal(impulse, np.eye(T)[T // 2 - 1]) and not np.signbit(impulse).any()
    # the taps delay by T/2 - 1 + f: a slow sine through them lags by that much
    T, f = 32, 0.25
    n = np.arange(400, dtype=np.float64)
    y = np.convolve(np.sin(0.05 * n), pkg.blend_fraction_taps(T, f))[:400]
    assert np.max(np.abs(y[T:] - np.sin(0.05 * (n[T:] - (T // 2 - 1 + f))))) < 1e-4
    for T, f in ((3, 0.5), (0, 0.5), (66, 0.5), (8, 1.0), (8, -0.25), (8, float("nan"))):
        with pytest.raises(pkg.GdgError, match="blend fraction taps") as e:
            pkg.blend_fraction_taps(T, f)
        assert e.value.code == pkg.GDG_ERR_INVALID


def test_the_library_s_fraction_planner_is_the_restatement_on_random_records(pkg):
    rng = np.random.default_rng(78)
    for steps in (1, 2, 3, 4):
        K, fits, blocks = 2 * steps - 1, 9, 5
        rec = np.zeros((fits, blocks), dtype=pkg.FIT_DTYPE)
        rec["terms"] = K
        rec["tt"] = rng.uniform(0.0, 2.0, (fits, blocks))
        rec["tt"][3] = 0.0                                                         # a silent target
        for k in range(K):
            rec["tx"][:, :, k] = rng.uniform(-1.0, 1.0, (fits, blocks))
            rec["xx"][:, :, k * (k + 1) // 2 + k] = rng.choice([0.0, 0.5, 2.0], (fits, blocks))
        rec["xx"][5] = 0.0                                                         # every candidate silent
        rec["tx"][6] = np.round(rec["tx"][6], 1)
        rec["xx"][6] = np.where(rec["xx"][6] > 0, 1.0, 0.0)                        # coarse values: ties
        got = pkg.blend_fractions_from_fit(rec, steps)
        want = [ref.fraction_step(rec[f], steps) for f in range(fits)]
        assert got == want and got[3] == 0 and got[5] == 0 and all(-(steps - 1) <= s <= steps - 1 for s in got), (steps, got, want)
    rec["terms"][2, 1] = 5
    with pytest.raises(pkg.GdgError, match="fit 2") as e:
        pkg.blend_fractions_from_fit(rec, 4)
    assert e.value.code == pkg.GDG_ERR_INVALID
    rec["terms"][2, 1] = 7
    rec["tx"][7, 0, 0] = np.inf
    with pytest.raises(pkg.GdgError, match="fit 7"):
        pkg.blend_fractions_from_fit(rec, 4)
    with pytest.raises(pkg.GdgError, match="steps = 5"):
        pkg.blend_fractions_from_fit(rec, 5)
