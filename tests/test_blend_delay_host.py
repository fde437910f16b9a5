"""The CPU side of the delayed blend outputs (gdg_batch_set_blends_delayed, gdg_blend_rows_delayed, gdg_blend_delays_from_align):
csrc/blend.h -- the refusal of a delay out of range, the list with delays as it replaces the one in force and is packed, the delayed sum on
the host against the known answer of include/gdg.h, and the planner on hand-made alignment records -- compiled without HIP into a
stand-alone program under AddressSanitizer and UBSan, run directly; then the planner through the library's own entry point against the
restatement (tests/blend_delay_ref.py).  What the kernels write is tests/test_gpu_blend_delay.py's business."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import blend_delay_ref as ref

ROOT = entry.ROOT


@pytest.fixture(scope="module")
def delay_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blend_delay") / "blend_delay_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "go-dsp-guitar_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "blend_delay_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_refusals_the_known_answer_and_the_planner_under_the_sanitizers(delay_check):
    r = subprocess.run([delay_check], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr


def test_the_restatement_gives_the_first_difference():
    x = np.array([[0.5, -0.25, 3.0, 3.0, -0.0, 1e-300]])
    got = ref.blend(x, [(0, 1.0, 0), (0, -1.0, 1)])
    assert np.array_equal(got, np.concatenate([x[0, :1], np.diff(x[0])])) and got[0] == x[0, 0] - 0.0
    hist = np.full((1, ref.MAX_DELAY), 7.0)
    hist[0, -1], hist[0, 0] = 2.0, -4.0
    assert ref.blend(x, [(0, 1.0), (0, -1.0, 1)], hist)[0] == -1.5
    assert np.array_equal(ref.blend(x, [(0, 1.0), (0, -1.0, ref.MAX_DELAY)], hist)[:2], [4.5, -7.25])
    assert ref.same_bits(ref.blend(x, [(0, 0.5), (0, 2.0)]), 0.5 * x[0] + 2.0 * x[0])      # no delay: the blend of tests/blend_ref.py


def test_the_library_s_planner_is_the_restatement_on_random_records():
    pkg = entry.load_package()
    pkg.build()
    rng = np.random.default_rng(77)
    ports, blocks = 6, 9
    rec = np.zeros((ports, blocks), dtype=pkg.BLOCK_ALIGN_DTYPE)
    rec["ref_sq"] = rng.choice([0.0, 4.0, 9.0], (ports, blocks), p=[0.15, 0.45, 0.4])
    rec["sq_at_lag"] = rng.choice([0.0, 1.0, 16.0], (ports, blocks), p=[0.15, 0.45, 0.4])
    rec["corr"] = rng.uniform(-1.0, 1.0, (ports, blocks)) * np.sqrt(rec["ref_sq"] * rec["sq_at_lag"])
    rec["lag"] = rng.integers(-2048, 2049, (ports, blocks))
    refs = [-1, 0, 0, 0, 4, 4]
    blends = [[(0, 1.0), (1, 0.5), (3, 0.25)], [(2, 1.0), (1, 1.0)], [(5, 1.0), (4, -1.0)], [(3, 2.0)]]
    for min_coeff in (0.0, 0.3, 0.6, 1.0):
        delays, signs = pkg.blend_delays_from_align(rec, refs, blends, min_coeff)
        for b, terms in enumerate(blends):
            roots = {refs[c] for c, _ in terms if refs[c] not in (-1, c)}
            root = roots.pop() if roots else terms[0][0]
            lag_sign = [(0, 1) if c == root else ref.port_lag(rec[c], min_coeff) for c, _ in terms]
            most = max(l for l, _ in lag_sign)
            assert delays[b] == [most - l for l, _ in lag_sign] and signs[b] == [s for _, s in lag_sign], (min_coeff, b)
            assert min(delays[b]) == 0 and max(delays[b]) <= ref.MAX_DELAY
    # mixed references: refused, the blend named
    with pytest.raises(pkg.GdgError, match="blend 1") as e:
        pkg.blend_delays_from_align(rec, refs, [[(0, 1.0), (1, 1.0)], [(1, 1.0), (4, 1.0)]], 0.5)
    assert e.value.code == pkg.GDG_ERR_INVALID
    with pytest.raises(pkg.GdgError, match="min_coeff"):
        pkg.blend_delays_from_align(rec, refs, blends, 1.5)
