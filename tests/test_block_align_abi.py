"""The CPU side of the alignment report (include/gdg.h, gdg_block_align_rows): the record's layout in C (compiled from the header) and in
BLOCK_ALIGN_DTYPE, the four entry points in every layer, the definition's known answers in its numpy restatement (tests/align_ref.py),
the wrapper's refusals, and the kernel's scratch and LDS from the compiler's own summary against the figure DESIGN.md states.  What the
kernel computes is tests/test_gpu_block_align.py's business."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import align_ref as ref

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
NAMES = ("gdg_block_align_rows", "gdg_block_align_rows_device", "gdg_batch_align_enable", "gdg_batch_align")
LAYOUT = (("corr", 0, 8), ("corr0", 8, 8), ("ref_sq", 16, 8), ("sq_at_lag", 24, 8), ("lag", 32, 4), ("reserved", 36, 4))


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_record_layout_in_c_and_in_numpy(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gdg.h"\nint main(void) {\n    printf("%zu", sizeof(gdg_block_align));\n' +
                   "".join('    printf(" %%zu %%zu", offsetof(gdg_block_align, %s), sizeof(((gdg_block_align *)0)->%s));\n' % (n, n) for n, _, _ in LAYOUT) +
                   '    printf("\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=300)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got == [40] + [v for _, off, size in LAYOUT for v in (off, size)]
    for dt in (pkg.BLOCK_ALIGN_DTYPE, ref.DTYPE):
        assert dt.itemsize == 40 and dt.names == tuple(n for n, _, _ in LAYOUT)
        assert [(dt.fields[n][1], dt.fields[n][0].itemsize) for n, _, _ in LAYOUT] == [(off, size) for _, off, size in LAYOUT]
        assert dt["lag"] == np.dtype("<i4") and dt["reserved"] == np.dtype("<u4") and dt["corr"] == np.dtype("<f8")


def test_header_carries_the_prototypes_and_the_library_exports_them(pkg):
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = " ".join(f.read().split())
    for proto in ("int gdg_block_align_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, const int *ref, int max_lag, "
                  "gdg_block_align *records);",
                  "int gdg_block_align_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, const int *ref, "
                  "int max_lag, gdg_block_align *d_records);",
                  "int gdg_batch_align_enable(gdg_ctx *ctx, const int *ref, int n_ports, int max_lag);",
                  "int gdg_batch_align(gdg_ctx *ctx, gdg_block_align *records, size_t capacity, int *ports, size_t *blocks);"):
        assert proto in header, proto
    for phrase in ("r[l] = sum_{n = M}^{L-M-1} x[n] * y[n + l]", "1 <= M <= 2048", "the smaller |l|, then the negative one", "p arrives LATER than its reference"):
        assert phrase in header, phrase
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for n in NAMES:
        assert n in exported and n in pkg.ABI_SYMBOLS and getattr(pkg.lib(), n).argtypes is not None, n
    for m in ("block_align", "block_align_device", "batch_align_enable", "batch_align"):
        assert callable(getattr(pkg.Context, m)), m
    base = os.path.dirname(os.path.dirname(pkg.LIB_PATH))
    with open(os.path.join(base, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    for fn, sym in zip(("BlockAlignRows", "BlockAlignRowsDevice", "BatchAlignEnable", "BatchAlign"), NAMES):
        assert re.search(r"^func \(this \*Context\) %s\(" % fn, go, re.M) and "C.%s(" % sym in go, fn
    assert re.search(r"^type BlockAlign struct", go, re.M)


def test_known_answers_hold_in_the_restatement():
    """an impulse against a shifted, scaled impulse; the sign of the lag; silence; a row against itself; the tie rule; non-finite samples"""
    for M in (1, 64, 2048):
        x = np.zeros(ref.L)
        x[4000] = 1.0
        for d in (0, 1, -1, M, -M):
            y = np.zeros(ref.L)
            y[4000 + d] = -2.0
            rec, r, y_sq = ref.record(x, y, M)
            assert (rec["lag"], rec["corr"], rec["ref_sq"], rec["sq_at_lag"], y_sq) == (d, -2.0, 1.0, 4.0, 4.0) and rec["corr0"] == (-2.0 if d == 0 else 0.0)
            assert r.size == 2 * M + 1 and ref.margin(r, M) == 2.0
    rec, r, _ = ref.record(np.zeros(100), np.zeros(100), 64)
    assert rec == dict(corr=0.0, corr0=0.0, ref_sq=0.0, sq_at_lag=0.0, lag=0, reserved=0)
    noise = np.random.default_rng(3).standard_normal(ref.L)
    rec, _, _ = ref.record(noise, noise, 2048)
    assert rec["lag"] == 0 and rec["corr"] == rec["ref_sq"] == rec["sq_at_lag"] == rec["corr0"]
    # equal magnitudes: the smaller |l|, then the negative one
    assert ref.pick(np.array([1.0, 0.0, -1.0, 0.0, 1.0]), 2) == 0 and ref.pick(np.array([3.0, 1.0, 0.0, 1.0, -3.0]), 2) == -2
    assert ref.pick(np.array([0.0, 2.0, 0.0, -2.0, 0.0]), 2) == -1 and ref.pick(np.zeros(5), 2) == 0
    # outside the central slice the reference does not count; a sample outside the block of p is never met
    x = np.zeros(ref.L)
    x[10] = 5.0
    rec, _, _ = ref.record(x, x, 64)
    assert rec["ref_sq"] == 0.0 and rec["corr"] == 0.0 and rec["lag"] == 0
    bad = np.array([0.25, np.nan, -0.5, np.inf, -np.inf] + [0.0] * 95)
    assert ref.record(bad, bad, 1)[0] == ref.record(np.where(np.isfinite(bad), bad, 0.0), np.where(np.isfinite(bad), bad, 0.0), 1)[0]
    recs = ref.block_align([noise, -noise], [-1, 0], 64)
    assert recs.shape == (2, 1) and recs[0, 0].tobytes() == bytes(40) and recs[1, 0]["corr"] < 0.0 and recs[1, 0]["lag"] == 0


@pytest.mark.parametrize("refs,max_lag", [([0, 2], 64), ([-2, 0], 64), ([0, 0], 0), ([0, 0], 2049), ([], 64)])
def test_the_wrapper_refuses_bad_lists_before_any_call(pkg, refs, max_lag):
    with pytest.raises(ValueError):
        pkg.align_refs(refs, max_lag)
    ghost = object.__new__(pkg.Context)                              # a context that was never created: any call through it would fail otherwise
    with pytest.raises(ValueError):
        pkg.Context.block_align(ghost, np.zeros((max(len(refs), 1), 16)), refs, max_lag)
    if refs:
        with pytest.raises(ValueError):
            pkg.Context.batch_align_enable(ghost, refs, max_lag)
    assert pkg.align_refs([0, -1, 1], 2048).dtype == np.int32


def test_the_c_calls_refuse_no_context(pkg):
    r = np.array([0, 0], dtype=np.int32)
    assert pkg.lib().gdg_batch_align_enable(None, r.ctypes.data, 2, 64) == pkg.GDG_ERR_INVALID
    assert pkg.lib().gdg_batch_align(None, None, 0, None, None) == pkg.GDG_ERR_INVALID
    assert pkg.lib().gdg_block_align_rows(None, None, 0, 0, r.ctypes.data, 64, None) == pkg.GDG_ERR_INVALID
    assert pkg.lib().gdg_block_align_rows_device(None, None, 0, 0, 0, r.ctypes.data, 64, None) == pkg.GDG_ERR_INVALID


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_kernel_uses_no_scratch_and_the_lds_design_md_states(tmp_path):
    """512 threads, one workgroup per CU: 2 waves per SIMD, so at most 256 vector registers; no scratch; LDS exactly what DESIGN.md 4.11b
    states, which is below 160 KiB"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        m = re.search(r"### 4\.11b.*?([\d ]+) bytes of LDS", f.read(), re.S)
    assert m, "DESIGN.md 4.11b states the kernel's LDS bytes"
    stated = int(m.group(1).replace(" ", ""))
    assert stated <= 160 * 1024
    out = str(tmp_path / "fir.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "fir.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @.*?^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        if "block_align_kernel" in m.group(1):
            found[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4))
    assert len(found) == 2, sorted(found)                            # pair loads and single loads
    for name, (vgprs, scratch, lds) in found.items():
        assert vgprs <= 256 and scratch == 0 and lds <= stated, (name, vgprs, scratch, lds)
