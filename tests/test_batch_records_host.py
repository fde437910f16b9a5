"""The C++ twin's one table of the nine record kinds a batch call keeps (host/batch_records.h): compiled without libgdg, HIP or the
Engine into a stand-alone program, plain and under AddressSanitizer and UBSan, and run against stub getters that serve known shapes
(tests/native/batch_records_check.cpp states what it holds).  No GPU: that the engine files every kind into its own store beside the
eight others is tests/test_host_mirror_batch_all_records.py's business."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
HOST = os.path.join(ROOT, "go-dsp-guitar_amd", "host")


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined"]], ids=["plain", "sanitized"])
def records_check(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("batch_records") / "batch_records_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + request.param +
                   ["-I", HOST, os.path.join(ROOT, "tests", "native", "batch_records_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_the_table_serves_all_nine_kinds_as_the_nine_copies_did(records_check):
    r = subprocess.run([records_check], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"OK (\d+) cases over 9 kinds\n", r.stdout)
    assert m, r.stdout + r.stderr
    # the nine kinds, the typed faces, the list without a block, the four port kinds over shards, and 74 on/off masks of a job without a block
    assert int(m.group(1)) >= 9 + 1 + 1 + 4 + 74


def test_the_header_stands_alone_and_the_engine_keeps_no_copy():
    """batch_records.h includes include/gdg.h and the standard library, nothing else; the engine's sources hold none of the per-kind
    members and helpers the table replaced, and the Makefile rebuilds the library with the header."""
    with open(os.path.join(HOST, "batch_records.h")) as f:
        header = f.read()
    includes = re.findall(r'^#include\s+(\S+)', header, re.M)
    assert [i for i in includes if i.startswith('"')] == ['"../../include/gdg.h"'] and all(re.fullmatch(r"<[a-z_]+>", i) for i in includes if not i.startswith('"'))
    code = re.sub(r"/\*.*?\*/|//[^\n]*", "", header, flags=re.S)           # the comments may name the Engine; the code may not
    assert not re.search(r"\bEngine\b|\bhip[A-Z]\w+\(", code)
    for name in ("gdg_host.cpp", "gdg_host.hpp"):
        with open(os.path.join(HOST, name)) as f:
            text = f.read()
        for word in ("lastReport_", "lastSpectrum_", "lastAlign_", "lastTruePeak_", "lastFit_", "lastGram_", "lastTapFit_", "lastTransfer_", "lastDelivered_",
                     "reportValid_", "deliveredValid_", "kindOf", "kindInto", "alignOf", "spectrumOf", "truePeakOf"):
            assert not re.search(r"\b%s\b" % word, text), "%s still names %s" % (name, word)
    with open(os.path.join(HOST, "Makefile")) as f:
        rule = [line for line in f if line.startswith("$(OUT):")]
    assert len(rule) == 1 and "batch_records.h" in rule[0].split()
