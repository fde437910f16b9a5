"""CPU side of the render report (gdg_block_stats, gdg_block_stats_rows / _rows_device, gdg_batch_report_enable, gdg_batch_report): the
record's layout as a C compiler sees it in include/gdg.h against the numpy dtype of the Python layer, the four entry points exported and
known to the Python layer, the Go binding and the C++ twin.  What the kernel computes is tests/test_gpu_block_stats.py's business."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
NAMES = ["gdg_block_stats_rows", "gdg_block_stats_rows_device", "gdg_batch_report_enable", "gdg_batch_report"]
FIELDS = [("peak", 0, 8), ("sum_sq", 8, 8), ("peak_index", 16, 4), ("clipped", 20, 4), ("full_scale", 24, 4), ("nonfinite", 28, 4)]

C_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "gdg.h"
typedef char size_is_32[sizeof(gdg_block_stats) == 32 ? 1 : -1];
typedef char peak_at_0[offsetof(gdg_block_stats, peak) == 0 ? 1 : -1];
typedef char sum_sq_at_8[offsetof(gdg_block_stats, sum_sq) == 8 ? 1 : -1];
typedef char peak_index_at_16[offsetof(gdg_block_stats, peak_index) == 16 ? 1 : -1];
typedef char clipped_at_20[offsetof(gdg_block_stats, clipped) == 20 ? 1 : -1];
typedef char full_scale_at_24[offsetof(gdg_block_stats, full_scale) == 24 ? 1 : -1];
typedef char nonfinite_at_28[offsetof(gdg_block_stats, nonfinite) == 28 ? 1 : -1];
int main(void) {
    gdg_ctx *ctx = NULL;
    gdg_block_stats rec[2];
    const double row[4] = { 0.0, 0.5, -1.0, 2.0 };
    const double *rows[1];
    int ports = 0, r[4];
    size_t blocks = 0;
    rows[0] = row;
    r[0] = gdg_block_stats_rows(ctx, rows, 1, 4, 2, rec);
    r[1] = gdg_block_stats_rows_device(ctx, row, 4, 1, 4, 2, rec);
    r[2] = gdg_batch_report_enable(ctx, 1);
    r[3] = gdg_batch_report(ctx, rec, 2, &ports, &blocks);
    printf("%d %d %d %d\n", r[0], r[1], r[2], r[3]);
    printf("%u", (unsigned)sizeof(gdg_block_stats));
    printf(" %u %u", (unsigned)offsetof(gdg_block_stats, peak), (unsigned)sizeof(rec[0].peak));
    printf(" %u %u", (unsigned)offsetof(gdg_block_stats, sum_sq), (unsigned)sizeof(rec[0].sum_sq));
    printf(" %u %u", (unsigned)offsetof(gdg_block_stats, peak_index), (unsigned)sizeof(rec[0].peak_index));
    printf(" %u %u", (unsigned)offsetof(gdg_block_stats, clipped), (unsigned)sizeof(rec[0].clipped));
    printf(" %u %u", (unsigned)offsetof(gdg_block_stats, full_scale), (unsigned)sizeof(rec[0].full_scale));
    printf(" %u %u\n", (unsigned)offsetof(gdg_block_stats, nonfinite), (unsigned)sizeof(rec[0].nonfinite));
    return 0;
}
"""


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_the_record_is_32_bytes_with_the_six_offsets_and_the_calls_link(pkg, tmp_path):
    """the probe's typedefs refuse to compile if the size or an offset is off; what it prints is compared again here"""
    src = tmp_path / "block_stats_probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "block_stats_probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    status, layout = r.stdout.strip().split("\n")
    assert [int(v) for v in status.split()] == [pkg.GDG_ERR_INVALID] * 4            # no context: refused, nothing touched
    numbers = [int(v) for v in layout.split()]
    assert numbers[0] == 32
    assert list(zip(numbers[1::2], numbers[2::2])) == [(off, size) for _, off, size in FIELDS]


def test_the_numpy_dtype_has_the_same_layout(pkg):
    dt = pkg.BLOCK_STATS_DTYPE
    assert dt.itemsize == 32 and dt.names == tuple(name for name, _, _ in FIELDS)
    for name, off, size in FIELDS:
        sub, at = dt.fields[name][:2]
        assert (at, sub.itemsize) == (off, size), name
        assert sub.byteorder in ("<", "=", "|") and sub == np.dtype("<f8" if size == 8 else "<u4"), name
    # a record written field by field reads back from its 32 little-endian bytes
    rec = np.zeros(1, dtype=dt)
    rec[0] = (0.5, 0.25, 7, 1, 2, 3)
    raw = rec.tobytes()
    assert raw == np.array([0.5, 0.25], dtype="<f8").tobytes() + np.array([7, 1, 2, 3], dtype="<u4").tobytes()


def test_the_header_declares_them_and_states_the_summation_rule():
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        text = f.read()
    for name in NAMES:
        assert re.search(r"^int %s\(gdg_ctx \*ctx" % name, text, re.M), name
    assert re.search(r"typedef struct \{[^}]*\bpeak\b[^}]*\bsum_sq\b[^}]*\bpeak_index\b[^}]*\bclipped\b[^}]*\bfull_scale\b[^}]*\bnonfinite\b[^}]*\} gdg_block_stats;", text)
    assert "depends on the block's LENGTH and on nothing else" in text and "not part of a checkpoint" in text
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "gdg.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_library_exports_them_and_every_layer_knows_them(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert name in exported, name
        assert name in pkg.ABI_SYMBOLS, name
        assert getattr(pkg.lib(), name).argtypes is not None
    for meth in ("block_stats", "batch_report_enable", "batch_report"):
        assert callable(getattr(pkg.Context, meth))
    base = os.path.dirname(os.path.dirname(pkg.LIB_PATH))
    with open(os.path.join(base, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    for fn, c in (("BlockStatsRows", "gdg_block_stats_rows"), ("BlockStatsRowsDevice", "gdg_block_stats_rows_device"),
                  ("BatchReportEnable", "gdg_batch_report_enable"), ("BatchReport", "gdg_batch_report")):
        assert re.search(r"^func \(this \*Context\) %s\(" % fn, go, re.M), fn
        assert "C.%s(" % c in go, c
    assert re.search(r"^type BlockStats struct", go, re.M)
    with open(os.path.join(base, "host", "gdg_host.hpp")) as f:
        hpp = f.read()
    with open(os.path.join(base, "host", "gdg_host.cpp")) as f:
        cpp = f.read()
    assert "void SetBatchReport(bool on)" in hpp and re.search(r"Error LastBatchReport\(", hpp)
    assert re.search(r"^Error Engine::LastBatchReport\(", cpp, re.M) and "gdg_batch_report_enable(" in cpp
    import inspect
    from go_dsp_guitar_amd import host
    for meth in ("batch_run", "batch_stream", "batch_stream_sharded"):
        assert inspect.signature(getattr(host.Engine, meth)).parameters["report"].default is False, meth
