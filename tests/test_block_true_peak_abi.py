"""The CPU side of the true-peak record (include/gdg.h, gdg_block_true_peak_rows): gdg_true_peak_taps against the formula (the library
loads without a device), the record's layout in C (compiled from the header) and in BLOCK_TRUE_PEAK_DTYPE, the five entry points in every
layer, the definition's known answers in its numpy restatement (tests/true_peak_ref.py), and the kernel's scratch, registers and LDS from
the compiler's own summary against what DESIGN.md states.  What the kernel computes is tests/test_gpu_block_true_peak.py's business."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import true_peak_ref as ref

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
NAMES = ("gdg_true_peak_taps", "gdg_block_true_peak_rows", "gdg_block_true_peak_rows_device", "gdg_batch_true_peak_enable", "gdg_batch_true_peak")
LAYOUT = (("true_peak", 0, 8), ("position", 8, 4), ("overs", 12, 4))
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_taps_against_the_formula(pkg):
    """each tap is at most six rounded operations plus two libm calls of <= 2 ulp, on values <= 1: 16 * 2^-52 absolute"""
    taps = pkg.true_peak_taps()
    assert taps.shape == (3, 24) and taps.dtype == np.float64
    assert np.max(np.abs(taps - ref.formula_taps())) <= 16 * EPS
    for p in range(3):
        s = 0.0
        for v in taps[p]:
            s = s + v
        assert abs(s - 1.0) <= 24 * EPS, (p, s)
    assert np.max(np.abs(taps[0] - taps[2][::-1])) <= 24 * EPS, "phase 1 mirrors phase 3"
    assert np.max(np.abs(taps[1] - taps[1][::-1])) <= 24 * EPS, "phase 2 is symmetric"
    assert abs(taps[1][11] - 0.633825) < 1e-6 and abs(taps[1][12] - 0.633825) < 1e-6


def test_taps_refusals(pkg):
    lib = pkg.lib()
    room = np.full(80, -7.0)
    assert lib.gdg_true_peak_taps(None, 72) == pkg.GDG_ERR_INVALID
    assert lib.gdg_true_peak_taps(room.ctypes.data, 71) == pkg.GDG_ERR_INVALID and lib.gdg_true_peak_taps(room.ctypes.data, 0) == pkg.GDG_ERR_INVALID
    assert lib.gdg_true_peak_taps(room.ctypes.data, -1) == pkg.GDG_ERR_INVALID and np.all(room == -7.0)
    assert lib.gdg_true_peak_taps(room.ctypes.data, 72) == pkg.GDG_OK
    assert room[:72].tobytes() == pkg.true_peak_taps().tobytes() and np.all(room[72:] == -7.0)


def test_record_layout_in_c_and_in_numpy(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gdg.h"\nint main(void) {\n    printf("%zu", sizeof(gdg_block_true_peak));\n' +
                   "".join('    printf(" %%zu %%zu", offsetof(gdg_block_true_peak, %s), sizeof(((gdg_block_true_peak *)0)->%s));\n' % (n, n) for n, _, _ in LAYOUT) +
                   '    printf("\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, timeout=300)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout.split()]
    assert got == [16] + [v for _, off, size in LAYOUT for v in (off, size)]
    for dt in (pkg.BLOCK_TRUE_PEAK_DTYPE, ref.DTYPE):
        assert dt.itemsize == 16 and dt.names == tuple(n for n, _, _ in LAYOUT)
        assert [(dt.fields[n][1], dt.fields[n][0].itemsize) for n, _, _ in LAYOUT] == [(off, size) for _, off, size in LAYOUT]
        assert dt["true_peak"] == np.dtype("<f8") and dt["position"] == np.dtype("<u4") and dt["overs"] == np.dtype("<u4")


def test_header_carries_the_prototypes_and_the_library_exports_them(pkg):
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = " ".join(f.read().split())
    for proto in ("int gdg_true_peak_taps(double *taps, int capacity);",
                  "int gdg_block_true_peak_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, gdg_block_true_peak *records);",
                  "int gdg_block_true_peak_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, "
                  "gdg_block_true_peak *d_records);",
                  "int gdg_batch_true_peak_enable(gdg_ctx *ctx, int enable);",
                  "int gdg_batch_true_peak(gdg_ctx *ctx, gdg_block_true_peak *records, size_t capacity, int *ports, size_t *blocks);"):
        assert proto in header, proto
    for phrase in ("23 intervals per block boundary", "0.633825", "0.900330", "a tie goes to the lower position", "price of statelessness"):
        assert phrase in header, phrase
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for n in NAMES:
        assert n in exported and n in pkg.ABI_SYMBOLS and getattr(pkg.lib(), n).argtypes is not None, n
    for m in ("block_true_peak", "block_true_peak_device", "batch_true_peak_enable", "batch_true_peak"):
        assert callable(getattr(pkg.Context, m)), m
    base = os.path.dirname(os.path.dirname(pkg.LIB_PATH))
    with open(os.path.join(base, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    assert re.search(r"^func TruePeakTaps\(", go, re.M) and "C.gdg_true_peak_taps(" in go
    for fn, sym in zip(("BlockTruePeakRows", "BlockTruePeakRowsDevice", "BatchTruePeakEnable", "BatchTruePeak"), NAMES[1:]):
        assert re.search(r"^func \(this \*Context\) %s\(" % fn, go, re.M) and "C.%s(" % sym in go, fn
    assert re.search(r"^type BlockTruePeak struct", go, re.M)
    with open(os.path.join(base, "host", "gdg_host.hpp")) as f:
        hpp = f.read()
    assert "SetBatchTruePeak(bool" in hpp and "LastBatchTruePeak(" in hpp
    with open(os.path.join(base, "csrc", "Makefile")) as f:
        make = f.read()
    assert re.search(r"^io\.o:.*true_peak_kernels\.h.*true_peak_taps\.h", make, re.M) and re.search(r"^api_%\.o:.*true_peak_taps\.h", make, re.M)


def test_the_c_calls_refuse_no_context(pkg):
    lib = pkg.lib()
    assert lib.gdg_batch_true_peak_enable(None, 1) == pkg.GDG_ERR_INVALID
    assert lib.gdg_batch_true_peak(None, None, 0, None, None) == pkg.GDG_ERR_INVALID
    assert lib.gdg_block_true_peak_rows(None, None, 1, 8, None) == pkg.GDG_ERR_INVALID
    assert lib.gdg_block_true_peak_rows_device(None, None, 8, 1, 8, None) == pkg.GDG_ERR_INVALID


def test_known_answers_hold_in_the_restatement(pkg):
    """the header's known answers, with the library's own taps and with the formula's"""
    n = np.arange(ref.L)
    for taps in (pkg.true_peak_taps(), ref.formula_taps()):
        x = np.zeros(ref.L)
        x[4000] = 1.0
        assert ref.record(x, taps) == (1.0, 16000, 0)
        _, v = ref.points(x, taps)
        assert abs(v[1][4000 - 11] - 0.633825) < 1e-6 and abs(v[1][3999 - 11] - 0.633825) < 1e-6
        peak, pos, overs = ref.record(np.full(ref.L, 0.5), taps)
        assert 0.5 <= peak <= 0.5 * (1 + 24 * EPS) and overs == 0
        s = 0.9 * np.sin(2 * np.pi * n / 4 + np.pi / 4)
        peak, pos, overs = ref.record(s, taps)
        assert abs(np.max(np.abs(s)) - 0.636396) < 1e-6 and abs(peak - 0.900330) < 1e-6 and pos % 4 == 2 and overs == 0
        assert ref.record(np.zeros(ref.L), taps) == (0.0, 0, 0) and ref.record(np.zeros(5), taps) == (0.0, 0, 0)
        # the gain of the three phases: |H_p(f)| = |sum_j h_p[j] exp(-2 pi i f j)|
        j = np.arange(-ref.H + 1, ref.H + 1)
        gain = lambda f: np.abs(np.array([np.sum(taps[p] * np.exp(-2j * np.pi * f * j)) for p in range(3)]))
        for f in np.linspace(0.0, 0.35, 141):
            assert np.all(np.abs(gain(f) - 1.0) <= (5e-4 if f <= 0.25 else 1.5e-3)), f
        assert abs(gain(0.25)[1] - 1.000366) < 1e-6 and abs(gain(1.0 / 3.0)[1] - (1.0 + 1.46e-3)) < 1e-5
        assert abs(gain(0.4)[1] - 1.005) < 1e-3 and abs(gain(0.45)[1] - 0.9) < 1e-3
        # a short block: fewer than 24 samples has no interpolated point; exactly 24 has one interval
        short = np.full(23, -0.75)
        assert ref.record(short, taps) == (0.75, 0, 0)
        assert ref.points(np.ones(24), taps)[1].shape == (3, 1)
        # non-finite samples count as 0; a negative crest; a tie goes to the lower position
        bad = np.zeros(100)
        bad[[3, 50, 70]] = np.nan, np.inf, -np.inf
        assert ref.record(bad, taps) == (0.0, 0, 0)
        two = np.zeros(ref.L)
        two[[1000, 5000]] = -0.75
        assert ref.record(two, taps) == (0.75, 4000, 0)
    recs = ref.block_true_peak([np.full(ref.L + 1, 0.25)], ref.formula_taps())
    assert recs.shape == (1, 2) and recs[0, 1]["true_peak"] == 0.25 and recs[0, 1]["position"] == 0


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_kernel_uses_no_scratch_and_leaves_two_workgroups_per_cu(tmp_path):
    """256 threads, two workgroups per CU: LDS at most 80 KiB and exactly what DESIGN states, no scratch, at most 256
    vector registers (2 waves per SIMD); and no fused multiply-add of doubles anywhere in the kernel"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    m = re.search(r"### 4\.11c.*?(\d+) vector registers.*?([\d ]+) bytes of LDS", design, re.S)
    assert m, "DESIGN.md 4.11c states the kernel's registers and LDS bytes"
    stated_vgprs, stated = int(m.group(1)), int(m.group(2).replace(" ", ""))
    assert 2 * stated <= 160 * 1024
    out = str(tmp_path / "io.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "io.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @(.*?)^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        if "block_true_peak_kernel" in m.group(1):
            found[m.group(1)] = tuple(int(m.group(i)) for i in (3, 4, 5)) + (m.group(2).count("v_fma_f64"), m.group(2).count("v_mul_f64"))
    assert len(found) == 2, sorted(found)                            # pair loads and single loads
    for name, (vgprs, scratch, lds, fma, mul) in found.items():
        assert vgprs <= stated_vgprs <= 256 and scratch == 0 and lds == stated and fma == 0 and mul >= 72, (name, vgprs, scratch, lds, fma, mul)
