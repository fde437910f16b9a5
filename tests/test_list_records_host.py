"""The list records (blend fit, Gram list, tap fit) under one path, without a GPU: the copy rule of their host stores as a stand-alone
program (tests/native/list_file_check.cpp), built plainly and once more under AddressSanitizer and UBSan; the one chain of the five
kinds' sections against the rule it replaced (tests/native/list_chain_check.cpp), built the same two ways; and the source text: the three
copies of the section arithmetic are gone from csrc/, and each of the three shard refusals is worded in one place."""
import glob
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry
import list_chain_pins

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
REMOVED = ["fit_section", "fit_room", "gram_section", "gram_room", "tapfit_section", "tapfit_room", "FitSection", "GramSection", "TapFitSection"]
SHARD_REFUSALS = ["a sharded job cannot collect fit records yet", "a sharded job cannot collect Gram records yet", "a sharded job cannot collect tap-fit records yet"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_the_host_stores_copy_rule_as_a_stand_alone_program(tmp_path, flags):
    exe = str(tmp_path / "list_file_check")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "list_file_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"OK list stores; (\d+) cases\n", r.stdout)
    assert m, r.stdout + r.stderr
    # rows in {1, 3} x element sizes {368, a Gram of 3 ports, 10 doubles} x (w = 1 at b0 = 0, 1, 2 and w = 2 at b0 = 0, 1) in a store of 3 blocks
    assert int(m.group(1)) == 2 * 3 * 5


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_the_one_chain_of_five_sections_against_the_rule_it_replaced(tmp_path, flags):
    exe = str(tmp_path / "list_chain_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "list_chain_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"OK one chain; (\d+) cases, (\d+) sections behind an end off a 16-byte boundary\n", r.stdout)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) == 32 * 5 * 4 and int(m.group(2)) > 0                # 32 on/off masks x 5 step widths x 4 ends; the 16-byte step was taken
    assert not r.stderr, r.stderr                                                # a sanitizer's report


def csrc_text():
    text = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.splitext(path)[1] in (".h", ".cpp", ".hip") or os.path.basename(path) == "Makefile":
            with open(path) as f:
                text[os.path.basename(path)] = f.read()
    assert {"report_sections.h", "ctx.h", "api_batch.cpp", "api_io.cpp", "api_checkpoint.cpp"} <= set(text)
    return text


def test_the_three_copies_are_gone_and_every_shard_refusal_is_worded_once():
    text = csrc_text()
    for name in REMOVED:
        found = [f for f, t in text.items() if re.search(r"\b%s\b" % name, t)]
        assert not found, (name, found)
    for literal in SHARD_REFUSALS:
        assert sum(t.count(literal) for t in text.values()) == 1, literal
    # one layout, one store: the header states the kinds in the order they ride, the context keeps one store per kind
    list_chain_pins.assert_one_chain(CSRC)
    assert "enum { REPORT_STATS, REPORT_BANDS, REPORT_ALIGN, REPORT_TRUE_PEAK, REPORT_KINDS };" in text["report_sections.h"]      # ... and they are no report kinds
    assert "list_rec[LIST_KINDS]" in text["ctx.h"]
    for old in ("FitRecords", "GramRecords", "TapFitRecords", "fit_begin", "gram_begin", "tapfit_begin", "fit_file", "gram_file", "tapfit_file"):
        assert not any(re.search(r"\b%s\b" % old, t) for t in text.values()), old
    # the shard entry points, the resume among them, ask the one function
    calls = re.findall(r'lists_refused\(ctx, "(\w+)"\)', text["api_batch.cpp"] + text["api_checkpoint.cpp"])
    assert sorted(calls) == ["gdg_batch_run_shard", "gdg_batch_stream_open_shard", "gdg_batch_stream_resume_shard", "gdg_batch_stream_step_shard"], calls


def test_the_four_carried_histories_are_set_up_and_refused_in_one_place():
    """blend, delivery, the ratio's and the delivered rows': one helper allocates, refuses and zeroes; the refusal's words, which no call can
    provoke while gdg_batch_release refuses an open job, are what the four copies said"""
    batch = csrc_text()["api_batch.cpp"]
    assert batch.count('"the %s history of the open job is gone (gdg_batch_release between two slices?)"') == 1 and batch.count("is gone") == 1
    whose = re.findall(r'carried_history\(ctx, (\w+), [^"]*"([^"]*)"', batch)
    assert whose == [("BATCH_BLEND_HISTORY", "blend"), ("BATCH_DELIVER_HISTORY", "delivery"), ("BATCH_DELIVER_RATIO_HISTORY", "delivery ratio's"),
                     ("BATCH_DELIVERED_REC_HISTORY", "delivered rows'")], whose
    # ... and no free loop over the slots is written out beside batch_buffer's and batch_drop's own
    assert batch.count("hipFree(ctx->batch_dev[") == 2 and batch.count("batch_drop(ctx, {") >= 6


def test_the_layout_header_needs_no_hip_header(tmp_path):
    src = tmp_path / "only_sections.cpp"
    src.write_text('#include "report_sections.h"\nint main() { const ListShape s = { 1, 8 }; return (int)list_section(0, s, 1).at; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(tmp_path / "only_sections")], check=True, timeout=300)
    with open(os.path.join(CSRC, "report_sections.h")) as f:
        assert "hip" not in [w for line in f if line.startswith("#include") for w in re.split(r"[<>\"/ .]", line)]
