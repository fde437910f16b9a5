"""The delivered rows' records (include/gdg.h, DELIVERED RECORDS) in the C-ABI, without a GPU: the record's 40 bytes in C and in numpy, exports
equal prototypes, every layer knows the calls, the header compiles as pedantic C99 with the new calls in use, the planner against
gdg_trim_from_true_peak and what it refuses, and the kernels' scratch, registers and LDS from the compiler's own summary against DESIGN.md
4.12k.  What the kernel computes is tests/test_gpu_delivered.py's business."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import delivered_ref as ref

ROOT = entry.ROOT
CSRC = os.path.join(entry.PKG_DIR, "csrc")
NEW = ["gdg_block_out_rows", "gdg_block_out_rows_device", "gdg_batch_out_records_enable", "gdg_batch_out_records", "gdg_trim_from_out_records"]
LAYOUT = (("true_peak", 0, 8), ("peak", 8, 8), ("sum_sq", 16, 8), ("position", 24, 4), ("peak_index", 28, 4), ("overs", 32, 4), ("clipped", 36, 4))


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_record_layout_in_c_and_in_numpy(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gdg.h"\nint main(void) {\n    printf("%zu", sizeof(gdg_block_delivered));\n' +
                   "".join('    printf(" %%zu %%zu", offsetof(gdg_block_delivered, %s), sizeof(((gdg_block_delivered *)0)->%s));\n' % (n, n) for n, _, _ in LAYOUT) +
                   '    printf("\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=300)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got == [40] + [v for _, off, size in LAYOUT for v in (off, size)]
    for dt in (pkg.BLOCK_DELIVERED_DTYPE, ref.DTYPE):
        assert dt.itemsize == 40 and dt.names == tuple(n for n, _, _ in LAYOUT)
        assert [(dt.fields[n][1], dt.fields[n][0].itemsize) for n, _, _ in LAYOUT] == [(off, size) for _, off, size in LAYOUT]
        assert dt["position"] == np.dtype("<i4") and dt["true_peak"] == np.dtype("<f8")
    assert (pkg.DELIVERED_HISTORY, pkg.DELIVERED_MAX_BLOCK) == (ref.HISTORY, 16384)


def test_exports_equal_prototypes_and_every_layer_knows_them(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in exported and name in pkg.ABI_SYMBOLS and re.search(r"^int %s\(" % name, header, re.M), name
        assert getattr(pkg.lib(), name).argtypes is not None
    assert {n for n in exported if n.startswith("gdg_") and ("out_rows" in n or "out_records" in n)} == set(NEW)
    for method in ("batch_delivered_enable", "batch_delivered", "block_delivered_rows", "block_delivered_rows_device", "trim_from_delivered"):
        assert callable(getattr(pkg.Context, method)), method
    with open(os.path.join(entry.PKG_DIR, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    for name in NEW:
        assert "C.%s(" % name in go, name
    for fn in ("BlockDeliveredRows", "BlockDeliveredRowsDevice", "BatchDeliveredEnable", "BatchDelivered"):
        assert re.search(r"^func \(this \*Context\) %s\(" % fn, go, re.M), fn
    assert re.search(r"^func TrimFromDelivered\(", go, re.M) and re.search(r"^type BlockDelivered struct", go, re.M)
    with open(os.path.join(entry.PKG_DIR, "host", "gdg_host.hpp")) as f:
        hpp = f.read()
    assert "SetBatchDelivered(bool" in hpp and "LastBatchDelivered(" in hpp
    with open(os.path.join(entry.PKG_DIR, "host", "gdg_host.cpp")) as f:
        cpp = f.read()
    assert "gdgh_engine_set_batch_delivered(" in cpp and "gdgh_engine_last_batch_delivered(" in cpp
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("Interval n belongs to the block that holds sample n + 12", "The last 12 intervals of a job", "can be as low as -47", "position 400 and overs 0",
                   "position -2 and overs 1", "each 0.633825", "the hole this record closes", "A non-finite sample is taken as 0 everywhere", "BEFORE the trim or blend gain",
                   "the greater magnitude, then the lower signed position"):
        assert phrase in flat, phrase
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert re.search(r"^io\.o:.*delivered_kernels\.h", f.read(), re.M)


C_PROBE = r"""
#include <stdio.h>
#include "gdg.h"
/* what cgo does with the header: compile it as C, link the new symbols by their plain names */
int main(void) {
    gdg_block_delivered rec[2] = { { 0.5, 0.4, 1.0, -2, 0, 0, 0 }, { 2.0, 1.5, 3.0, 7, 1, 1, 1 } };
    gdg_block_true_peak tp[2] = { { 0.5, 0, 0 }, { 2.0, 7, 1 } };
    double a[2], b[2], x[4] = { 0.0, 0.0, 0.0, 0.0 };
    const double *rows[1];
    size_t span[2] = { 0, 4 };
    int r1, r2, r3, r4, r5;
    rows[0] = x;
    r1 = gdg_trim_from_out_records(rec, 2, 1, 0.891250938, 4.0, a);
    r2 = gdg_trim_from_true_peak(tp, 2, 1, 0.891250938, 4.0, b);
    r3 = gdg_block_out_rows(NULL, rows, 1, 4, span, 1, NULL, rec);
    r4 = gdg_block_out_rows_device(NULL, x, 4, 1, 4, span, 1, NULL, rec);
    r5 = gdg_batch_out_records_enable(NULL, 1) + gdg_batch_out_records(NULL, NULL, 0, NULL, NULL);
    printf("%d %d %d|%d %d %d|%d %d\n", r1, r2, a[0] == b[0] && a[1] == b[1], r3, r4, r5, GDG_OUT_RECORDS_HISTORY, GDG_OUT_RECORDS_MAX_BLOCK);
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
    assert r.stdout.strip() == "0 0 1|%d %d %d|23 16384" % (inv, inv, 2 * inv)


def test_the_planner_is_the_true_peak_planner_on_this_record(pkg):
    rng = np.random.default_rng(7)
    peaks = rng.uniform(0.0, 3.0, (6, 9))
    peaks[2] = 0.0                                                           # a silent port: gain 1
    peaks[4] *= 1e-3                                                         # a quiet one: max_gain caps
    rec = np.zeros((6, 9), dtype=pkg.BLOCK_DELIVERED_DTYPE)
    rec["true_peak"] = peaks
    rec["peak"], rec["position"], rec["sum_sq"] = 7.0, -47, 1e9            # nothing else is read
    tp = np.zeros((6, 9), dtype=pkg.BLOCK_TRUE_PEAK_DTYPE)
    tp["true_peak"] = peaks
    for target, max_gain in ((10.0 ** (-1.0 / 20.0), 4.0), (0.5, 100.0)):
        got, want = pkg.trim_from_delivered(rec, target, max_gain), pkg.trim_from_true_peak(tp, target, max_gain)
        assert got.tobytes() == want.tobytes() and got[2] == 1.0 and (got[4] == max_gain or max_gain == 100.0)
    lib, gain = pkg.lib(), np.zeros(6)
    inv = pkg.GDG_ERR_INVALID
    assert lib.gdg_trim_from_out_records(None, 6, 9, 0.5, 4.0, gain.ctypes.data) == inv and b"trim from out records" in lib.gdg_last_error(None)
    assert lib.gdg_trim_from_out_records(rec.ctypes.data, 0, 9, 0.5, 4.0, gain.ctypes.data) == inv
    assert lib.gdg_trim_from_out_records(rec.ctypes.data, 6, 0, 0.5, 4.0, gain.ctypes.data) == inv and b"6 ports x 0 blocks" in lib.gdg_last_error(None)
    assert lib.gdg_trim_from_out_records(rec.ctypes.data, 6, 9, 0.5, 4.0, None) == inv
    assert lib.gdg_trim_from_out_records(rec.ctypes.data, 6, 9, 0.0, 4.0, gain.ctypes.data) == inv and b"target" in lib.gdg_last_error(None)
    bad = rec.copy()
    bad["true_peak"][3, 1] = np.nan
    with pytest.raises(pkg.GdgError, match="port 3 has a NaN true_peak"):
        pkg.trim_from_delivered(bad, 0.5, 4.0)
    assert lib.gdg_batch_out_records_enable(None, 1) == inv and lib.gdg_batch_out_records(None, None, 0, None, None) == inv


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_kernels_use_no_scratch_and_the_figures_of_the_table(tmp_path):
    """From the compiler's resource summary of io.hip (-O3, gfx950): block_delivered_kernel and delivered_history_save_kernel (C linkage: plain
    names) use no scratch; the record kernel's LDS is the tile with its lead-in, 2072 doubles, and the reduction's 160 bytes, whatever the
    block's length; registers and LDS are the figures DESIGN.md 4.12k records; every product and add on its own."""
    out = str(tmp_path / "io.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "io.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\w*delivered\w+)\n.*?^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    assert sorted(found) == ["block_delivered_kernel", "delivered_history_save_kernel"]
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    part = design[design.index("### 4.12k"):]
    table = {n: (int(v), int(s), int(lds.replace(" ", ""))) for n, v, s, lds in re.findall(r"^\| `(\w*delivered\w+)` \| (\d+) \| (\d+) \| ([\d ]+) \|", part, re.M)}
    assert found == table, (found, table)
    assert found["block_delivered_kernel"][1:] == (0, (24 + 2048) * 8 + 160) and found["block_delivered_kernel"][0] <= 128      # four waves per SIMD
    assert found["delivered_history_save_kernel"][1:] == (0, 0)
    kernel = re.search(r"^block_delivered_kernel:.*?\.amdhsa_kernel", text, re.S | re.M).group(0)
    assert "v_fma_f64" not in kernel and kernel.count("v_mul_f64") >= 72 and "v_add_f64" in kernel
    assert not re.search(r"global_atomic|flat_atomic|ds_\w*(add|max)_\w*rtn", kernel)
