"""csrc/align_map.h, the host side of the alignment report (include/gdg.h, gdg_batch_align_enable), through a stand-alone program under
AddressSanitizer and UBSan: good lists, out-of-range references, a lag range of 0 and of 2049, an empty list, a list that replaces the one
in force only when it is valid as a whole (all by hand in tests/native/align_check.cpp), and the program's verdict and launch lists for
lists given here against the rule restated in Python."""
import os
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
OK, COUNT, NULL, REF, LAG = range(5)


@pytest.fixture(scope="module")
def align_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("align") / "align_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "align_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def verdict(ref, max_lag):
    if not 1 <= max_lag <= 2048:
        return LAG, -1
    for p, q in enumerate(ref):
        if q < -1 or q >= len(ref):
            return REF, p
    return OK, -1


@pytest.mark.parametrize("max_lag,ref", [(64, [0, 0, 0]), (1, [-1, -1]), (2048, [3, 2, 1, 0]), (64, [0, 3, 0]), (64, [-2, 0]), (0, [0, 0]), (2049, [0, 0]),
                                         (2048, [0] * 500 + [-1] * 15), (7, [5] * 481)])
def test_host_code_under_sanitizers(align_check, max_lag, ref):
    r = subprocess.run([align_check, str(max_lag)] + [str(v) for v in ref], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
    words = r.stdout.split()
    want = verdict(ref, max_lag)
    assert (int(words[1]), int(words[2])) == want
    if want[0] == OK:
        pieces = [[tuple(int(v) for v in w.split(":")) for w in part.split()] for part in " ".join(words[3:]).split("|")] if words[3:] else []
        measured = [(p, q) for p, q in enumerate(ref) if q >= 0]
        assert [pq for piece in pieces for pq in piece] == measured
        assert all(len(piece) == 240 for piece in pieces[:-1]) and all(1 <= len(piece) <= 240 for piece in pieces)
