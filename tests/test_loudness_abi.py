"""The loudness records (include/gdg.h, LOUDNESS) in the C-ABI, without a GPU: exports equal prototypes, every layer knows the calls, the
constants are as stated, the header compiles as pedantic C99 with the new calls in use, the feature rides a path of its own, and the kernel's
scratch, registers and LDS from the compiler's own summary against DESIGN.md 4.12l.  What the kernel computes is
tests/test_gpu_loudness.py's business."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry
import loudness_ref as ref

ROOT = entry.ROOT
CSRC = os.path.join(entry.PKG_DIR, "csrc")
NEW = ["gdg_loudness_coefficients", "gdg_loudness_hops", "gdg_loudness_rows", "gdg_loudness_rows_device", "gdg_batch_loudness_enable", "gdg_batch_loudness",
       "gdg_loudness_from_hops", "gdg_trim_from_loudness"]


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_exports_equal_prototypes_and_every_layer_knows_them(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in exported and name in pkg.ABI_SYMBOLS and re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
        assert getattr(pkg.lib(), name).argtypes is not None
    assert {n for n in exported if n.startswith("gdg_") and "loudness" in n} == set(NEW)
    assert not [n for n in NEW if "deliver" in n]                            # two tests count the factor stage's exports by that word
    for method in ("batch_loudness_enable", "batch_loudness", "loudness_rows", "loudness_rows_device", "loudness_from_hops", "trim_from_loudness"):
        assert callable(getattr(pkg.Context, method)), method
    with open(os.path.join(entry.PKG_DIR, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    for name in NEW:
        assert "C.%s(" % name in go, name
    for fn in ("LoudnessRows", "LoudnessRowsDevice", "BatchLoudnessEnable", "BatchLoudness"):
        assert re.search(r"^func \(this \*Context\) %s\(" % fn, go, re.M), fn
    for fn in ("LoudnessFromHops", "TrimFromLoudness", "LoudnessHops", "LoudnessCoefficients"):
        assert re.search(r"^func %s\(" % fn, go, re.M), fn
    with open(os.path.join(entry.PKG_DIR, "host", "gdg_host.hpp")) as f:
        hpp = f.read()
    assert "SetBatchLoudness(bool" in hpp and "LastBatchLoudness(" in hpp
    with open(os.path.join(entry.PKG_DIR, "host", "gdg_host.cpp")) as f:
        cpp = f.read()
    assert "gdgh_engine_set_batch_loudness(" in cpp and "gdgh_engine_last_batch_loudness(" in cpp
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("1681.974450955533", "0.7071752369554196", "3.999843853973347", "38.13547087602444", "0.5003270373238773", "0.4996667741545416",
                   "reads -3.01 LUFS", "A hop that the job's end cuts is never emitted", "A silent port gives exactly +0.0", "GDG_LOUDNESS_STATE_DOUBLES = 7",
                   "not of the window, of how a streamed job is sliced, or of whether outputs are written", "above -70 LUFS and above -10 LU"):
        assert phrase in flat, phrase


def test_the_constants_and_the_path_of_its_own(pkg):
    assert (pkg.LOUDNESS_STATE_DOUBLES, pkg.LOUDNESS_TILE) == (ref.STATE_DOUBLES, ref.TILE) == (7, 8192)
    text = {}
    for name in os.listdir(CSRC):
        if name.endswith((".h", ".cpp", ".hip")) or name == "Makefile":
            with open(os.path.join(CSRC, name)) as f:
                text[name] = f.read()
    assert {"loudness.h", "loudness_kernels.h", "loudness.hip", "api_loudness.cpp"} <= set(text)
    # no entry in the report kinds, the list kinds or the batch_dev slots; no carried_history; the refusals worded in one function of its own
    assert "LOUD" not in text["report_sections.h"].upper()
    assert not re.search(r"BATCH_\w*LOUD", text["ctx.h"]) and "carried_history" not in text["api_loudness.cpp"]
    assert text["api_batch.cpp"].count("carried_history(ctx, ") == 4
    assert sum(t.count("the loudness records are on on this context (gdg_batch_loudness_enable)") for t in text.values()) == 1
    calls = re.findall(r'loudness_refused\(ctx, "?(\w+)"?,', text["api_batch.cpp"] + text["api_checkpoint.cpp"])
    assert sorted(calls) == ["checkpoint", "checkpoint", "gdg_batch_finish_master", "gdg_batch_finish_master_slice", "gdg_batch_run_shard", "gdg_batch_stream_open_shard",
                             "gdg_batch_stream_step_shard", "what"], calls
    # the block loop is joined by three calls
    for fn in ("loudness_slice_begin(", "loudness_step(", "loudness_slice_end("):
        assert text["api_batch.cpp"].count(fn) == 1, fn
    with open(os.path.join(entry.PKG_DIR, "host", "batch_records.h")) as f:
        assert "oudness" not in f.read()
    assert re.search(r"^loudness\.o:.*loudness_kernels\.h", text["Makefile"], re.M) and "loudness.o" in text["Makefile"].split("OBJS")[1].split("\n")[0]


C_PROBE = r"""
#include <stdio.h>
#include "gdg.h"
/* what cgo does with the header: compile it as C, link the new symbols by their plain names */
int main(void) {
    double c[10], rec[8] = { 4800.0, 4800.0, 4800.0, 4800.0, 0.0, 0.0, 0.0, 0.0 }, gain[2], integrated = 0.0, x[4] = { 0.0, 0.0, 0.0, 0.0 };
    int port[1] = { 0 }, capped[2], r1, r2, r3, r4, r5;
    r1 = gdg_loudness_coefficients(48000, c);
    r2 = gdg_loudness_from_hops(rec, 2, 4, 48000, port, NULL, 1, &integrated, NULL, NULL);
    r3 = gdg_trim_from_loudness(rec, 2, 4, 48000, -23.0, -1.0, NULL, 0, gain, capped);
    r4 = gdg_loudness_rows(NULL, x, 4, 1, 0, 4, 48000, NULL, NULL, rec, 8) + gdg_loudness_rows_device(NULL, x, 4, 1, 0, 4, 48000, NULL, NULL, rec, 8);
    r5 = gdg_batch_loudness_enable(NULL, 1) + gdg_batch_loudness(NULL, NULL, 0, NULL, NULL);
    printf("%d %d %d|%d %d|%d %d %.3f %.1f %d %d|%d %d\n", r1, r2, r3, r4, r5, (int)gdg_loudness_hops(48000, 0, 98304), (int)gdg_loudness_hops(44100, 4000, 500),
           integrated, gain[1], capped[0], c[5] == 1.0 && c[6] == -2.0, GDG_LOUDNESS_STATE_DOUBLES, GDG_LOUDNESS_TILE);
    return 0;
}
"""


def test_the_header_is_pedantic_c99_with_the_new_calls(pkg, tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    inv = pkg.GDG_ERR_INVALID
    assert r.stdout.strip() == "0 0 0|%d %d|20 1 -0.691 1.0 0 1|7 8192" % (2 * inv, 2 * inv)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_kernel_uses_no_scratch_and_the_figures_of_the_table(tmp_path):
    """From the compiler's resource summary of loudness.hip (-O3, gfx950): block_loudness_kernel uses no scratch; its LDS is the tile at a pitch
    of 33 doubles per chunk, the scan's two buffers and the cell sums; registers and LDS are the figures DESIGN.md 4.12l records; every product
    and sum on its own; no atomics."""
    out = str(tmp_path / "loudness.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "loudness.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\w+)\n.*?^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    assert sorted(found) == ["block_loudness_kernel"]
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    part = design[design.index("### 4.12l"):]
    table = {n: (int(v), int(s), int(lds.replace(" ", ""))) for n, v, s, lds in re.findall(r"^\| `(\w*loudness\w+)` \| (\d+) \| (\d+) \| ([\d ]+) \|", part, re.M)}
    assert found == table, (found, table)
    assert found["block_loudness_kernel"][1:] == (0, (256 * 33 + 2 * 256 * 4 + 256) * 8) and found["block_loudness_kernel"][0] <= 512
    kernel = re.search(r"^block_loudness_kernel:.*?\.amdhsa_kernel", text, re.S | re.M).group(0)
    assert "v_fma_f64" not in kernel and "v_mul_f64" in kernel and "v_add_f64" in kernel
    assert not re.search(r"global_atomic|flat_atomic|ds_\w*(add|max)_\w*rtn|scratch_", kernel)
