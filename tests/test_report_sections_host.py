"""The layout of the render report's four record kinds in a batch call's download half (csrc/report_sections.h): compiled without HIP
into a stand-alone program under AddressSanitizer and UBSan and held against a literal restatement of the offset cascade, the master
finish's packed offsets and the slice runner's room terms it replaced (tests/native/report_sections_check.cpp).  No GPU: that the batch
calls file every kind's bytes where the layout says is tests/test_gpu_report_sections.py's business."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")


@pytest.fixture(scope="module")
def sections_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("report_sections") / "report_sections_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "report_sections_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_the_header_gives_the_offsets_sizes_ends_and_rooms_it_replaced(sections_check):
    r = subprocess.run([sections_check], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"OK (\d+) cases; sections moved by the 16-byte step: (\d+) (\d+) (\d+) (\d+)\n", r.stdout)
    assert m, r.stdout + r.stderr
    # 16 sets of kinds x plain, shard, finish x N in {1, 3, 8, 512} x w in {1, 2, 4, 16} x 4 widths x 3 band counts, at the least
    assert int(m.group(1)) >= 16 * 3 * 4 * 4 * 4 * 3
    assert all(int(m.group(k)) > 0 for k in range(2, 6))


def test_the_layout_is_stated_once():
    """The host files take every offset from the header: none of the cascade's names is left, and the Makefile rebuilds them with it."""
    for name in os.listdir(CSRC):
        if not name.endswith((".h", ".cpp", ".hip")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for word in ("before_tp", "spec_at", "align_at", "tp_at"):
            assert not re.search(r"\b%s\b" % word, text), "%s still names %s" % (name, word)
    with open(os.path.join(CSRC, "Makefile")) as f:
        rule = [line for line in f if line.startswith("api_%.o:")]
    assert len(rule) == 1 and "report_sections.h" in rule[0].split()
