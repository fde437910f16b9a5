"""csrc/true_peak_taps.h, the host side of the true-peak record (include/gdg.h, gdg_true_peak_taps), through a stand-alone program under
AddressSanitizer and UBSan: the table's sums and symmetries, the copy and its refusals, the evaluated range for every block length from 0
to 30 and for 8192 (all by hand in tests/native/true_peak_check.cpp), and the program's table against the definition restated in numpy
and against the library's."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import true_peak_ref as ref

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
LENGTHS = list(range(0, 31)) + [8192]


@pytest.fixture(scope="module")
def words(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("true_peak") / "true_peak_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "true_peak_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe] + [str(v) for v in LENGTHS], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    return r.stdout.split()


def test_host_code_under_sanitizers_builds_the_table_of_the_definition(words):
    taps = np.array([float.fromhex(w) for w in words[1:73]]).reshape(3, 24)
    assert np.max(np.abs(taps - ref.formula_taps())) <= 16 * 2.0 ** -52
    pkg = entry.load_package()
    pkg.build()
    assert taps.tobytes() == pkg.true_peak_taps().tobytes(), "the library hands out the table this header builds"


def test_evaluated_range_for_every_short_length(words):
    got = [tuple(int(v) for v in w.split(":")) for w in words[73:]]
    assert got == [(n, ref.H - 1, max(0, n - 2 * ref.H + 1)) for n in LENGTHS]
    for n in LENGTHS:
        _, v = ref.points(np.zeros(n), ref.formula_taps())
        assert v.shape == (3, max(0, n - 23))
