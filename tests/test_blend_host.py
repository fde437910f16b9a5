"""The CPU side of the blend outputs (gdg_batch_set_blends, gdg_blend_rows): csrc/blend.h -- the validation of a blend list, the rule by
which a list replaces the one in force, and the sum with every product and every add rounded on its own -- compiled without HIP into a
stand-alone program under AddressSanitizer and UBSan and held against the known answer of include/gdg.h and a table this file makes with
the numpy restatement (tests/blend_ref.py).  What the kernel writes is tests/test_gpu_blend.py's business."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import blend_ref as ref

ROOT = entry.ROOT


@pytest.fixture(scope="module")
def blend_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("blend") / "blend_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "go-dsp-guitar_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "blend_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_the_restatement_and_the_header_give_the_known_answer(blend_check):
    r = subprocess.run([blend_check], capture_output=True, text=True, timeout=120)      # the header's own known answers and refusals
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    ones = np.ones((3, 4))
    assert np.array_equal(ref.blend(ones, [(0, 0.1), (1, 0.2), (2, 0.3)]), np.full(4, 0.6000000000000001))
    assert np.array_equal(ref.blend(ones, [(2, 0.3), (1, 0.2), (0, 0.1)]), np.full(4, 0.6))
    rows = np.array([[0.25, np.inf], [-3.0, 2.0]])
    assert np.array_equal(ref.blend(rows, [(1, -1.0)]), [3.0, -2.0])
    twice = ref.blend(rows, [(0, 0.0), (1, 0.5), (0, 2.0)])
    assert twice[0] == -1.0 and np.isnan(twice[1])                            # 0 * inf is NaN
    assert ref.same_bits([1.0, np.nan], [1.0, -np.nan]) and not ref.same_bits([0.0], [-0.0]) and not ref.same_bits([np.nan], [1.0])


def test_the_sum_equals_numpy_s_on_random_terms(blend_check, tmp_path):
    rng = np.random.default_rng(41)
    lines = []
    for K in [1, 2, 3, 5, 8, 31, 32] * 60:
        w = rng.choice([0.6, 0.4, -1.0, 0.1, 0.2, 0.3, 0.0, 1.0], K) * np.where(rng.random(K) < 0.5, 1.0, rng.uniform(-2.0, 2.0, K))
        x = rng.uniform(-1.5, 1.5, K) * np.where(rng.random(K) < 0.2, 1e-9, 1.0)
        if rng.random() < 0.1:
            x[rng.integers(K)] = rng.choice([np.inf, -np.inf, np.nan])
        s = ref.blend(x[:, None], [(k, w[k]) for k in range(K)])[0]
        lines.append(" ".join(["%d" % K] + ["%x" % int(np.float64(v).view(np.uint64)) for v in list(w) + list(x) + [s]]))
    table = tmp_path / "table.txt"
    table.write_text("\n".join(lines) + "\n")
    r = subprocess.run([blend_check, str(table)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "OK %d rows" % len(lines), r.stdout + r.stderr
