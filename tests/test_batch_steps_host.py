"""The step plan of the batch block loop (csrc/batch_steps.h: job_step, slice_steps, step_pieces), without a GPU: a stand-alone program
(tests/native/batch_steps_check.cpp) holds it against the rule it replaced, against the cover and nesting properties that make a sliced job
step like the one-call job, and against sequences derived by hand; built plainly and once more under AddressSanitizer and UBSan.  And the
header needs no HIP header."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_the_step_plan_as_a_stand_alone_program(tmp_path, flags):
    exe = str(tmp_path / "batch_steps_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "batch_steps_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"OK step plan; (\d+) cases\n", r.stdout)
    assert m, r.stdout + r.stderr
    # 5 windows x the slices [origin, origin + n) of every job of 1 to 64 blocks: job (job + 1) / 2 of them per job
    assert int(m.group(1)) == 5 * sum(job * (job + 1) // 2 for job in range(1, 65)) == 228800
    if len(flags) > 1:
        assert not r.stderr, r.stderr                                            # a sanitizer's report


def test_the_step_plan_header_needs_no_hip_header(tmp_path):
    src = tmp_path / "only_steps.cpp"
    src.write_text('#include "batch_steps.h"\nint main() { return (int)slice_steps(29, 13, 16, 8).size() - 5 + step_pieces(4, 8) - 4; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "only_steps")], check=True, timeout=300)
    assert subprocess.run([str(tmp_path / "only_steps")], timeout=60).returncode == 0
    with open(os.path.join(CSRC, "batch_steps.h")) as f:
        includes = [line.strip() for line in f if line.startswith("#include")]
    assert includes == ["#include <stddef.h>", "#include <vector>"], includes
