"""The trim entry points at the drop-in boundary, without a GPU: the new prototypes compile as pedantic C99 and link by their plain names,
libgdg.so exports them, header and exports stay set-equal, every layer knows the calls, and the compiler's own summary shows that the new
kernels use no scratch, no LDS, no atomics and no fused multiply-add."""
import ctypes
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
NEW = ["gdg_batch_set_trim", "gdg_wave_encode_trim", "gdg_wave_encode_trim_device", "gdg_trim_from_true_peak"]

C_PROBE = r"""
#include <stdio.h>
#include "gdg.h"
int main(void) {
    double x[4] = { 0.0, 0.25, -0.5, 1.0 }, g[2] = { 0.5, -1.0 }, gain[3] = { -1.0, -1.0, -1.0 };
    unsigned char out[32];
    gdg_block_true_peak rec[3] = { { 0.5, 0, 0 }, { 2.0, 0, 0 }, { 0.0, 0, 0 } };
    const uint64_t seed = 0xdeadbeefcafef00dULL, first = 0x10000000001ULL;
    int rc;
    printf("%d %d %d\n", gdg_batch_set_trim(NULL, g, 2, 1.0, 1.0, 1.0), gdg_wave_encode_trim(NULL, GDG_FMT_LPCM16, x, 4, 0.5, 1, seed, 3u, first, out),
           gdg_wave_encode_trim_device(NULL, GDG_FMT_IEEE64, x, 4, 0.5, 0, seed, 3u, first, out));
    rc = gdg_trim_from_true_peak(rec, 3, 1, 0.891250938, 4.0, gain);
    printf("%d %.9f %.9f %.1f\n", rc, gain[0], gain[1], gain[2]);
    rec[0].true_peak = 0.01;
    rc = gdg_trim_from_true_peak(rec, 1, 1, 0.891250938, 4.0, gain);
    printf("%d %.1f\n", rc, gain[0]);
    rc = gdg_trim_from_true_peak(rec, 1, 1, 0.0, 4.0, gain);
    printf("%d %s\n", rc, gdg_last_error(NULL));
    return 0;
}
"""


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_the_prototypes_are_pedantic_c99_and_link_from_c(pkg, tmp_path):
    src = tmp_path / "trim_probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "trim_probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert [int(v) for v in lines[0].split()] == [pkg.GDG_ERR_INVALID] * 3          # no context: refused, nothing touched
    assert lines[1] == "0 1.782501876 0.445625469 1.0"                              # the planner needs no context and no device: the header's known answers
    assert lines[2] == "0 4.0"
    assert lines[3].startswith("%d " % pkg.GDG_ERR_INVALID) and "target" in lines[3]


def test_the_symbols_are_exported_and_header_and_exports_stay_set_equal(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gdg_[a-z_0-9]+)\s*\(", header))
    for name in NEW:
        assert name in exported and name in declared and name in pkg.ABI_SYMBOLS, name
        assert getattr(pkg.lib(), name).argtypes is not None
    assert {n for n in exported if n.startswith("gdg_")} == declared == set(pkg.ABI_SYMBOLS)
    lib = ctypes.CDLL(pkg.LIB_PATH)
    assert all(hasattr(lib, n) for n in NEW)


def test_every_layer_knows_the_calls(pkg):
    for name in ("batch_set_trim", "wave_encode_trim", "wave_encode_trim_device"):
        assert callable(getattr(pkg.Context, name)), name
    assert callable(pkg.trim_from_true_peak)
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = f.read()
    assert re.search(r"^int gdg_batch_set_trim\(gdg_ctx \*ctx, const double \*chain_gain, int n, double master_left, double master_right, double metronome\);", header, re.M)
    assert re.search(r"^int gdg_trim_from_true_peak\(const gdg_block_true_peak \*records, int ports, size_t blocks, double target, double max_gain, double \*gain\);",
                     header, re.M)
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("ONE IEEE-754 double multiply", "fl(|g| peak), clamped to 1", "|g| true_peak <= 1 no sample of the file is clipped", "BEFORE the trim",
                   "{1.782501876, 0.445625469, 1.0}", "give {4.0}", "stat_batch_device_kib is unchanged"):
        assert phrase in flat, phrase
    base = os.path.dirname(os.path.dirname(pkg.LIB_PATH))
    with open(os.path.join(base, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    assert re.search(r"^func \(this \*Context\) BatchSetTrim\(chainGain \[\]float64, masterLeft float64, masterRight float64, metronome float64\) error", go, re.M)
    assert re.search(r"^func TrimFromTruePeak\(records \[\]\[\]BlockTruePeak, target float64, maxGain float64\) \(\[\]float64, error\)", go, re.M)
    for call in ("C.gdg_batch_set_trim(", "C.gdg_wave_encode_trim(", "C.gdg_wave_encode_trim_device(", "C.gdg_trim_from_true_peak("):
        assert call in go, call
    from go_dsp_guitar_amd import host
    for name in ("render_normalized", "_set_trim"):
        assert callable(getattr(host.Engine, name)), name
    with open(os.path.join(base, "host", "gdg_host.hpp")) as f:
        assert "Error SetBatchTrim(const std::vector<double> &chainGain" in f.read()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_trim_kernels_use_no_scratch(tmp_path):
    """Every instantiation of the five new kernels, from the compiler's resource summary: no scratch, no LDS, no atomics, and the product is
    a v_mul_f64 of its own -- no fused multiply-add of doubles anywhere in them.  50 instantiations: the rows kernel and the two
    stand-alone ones in six plain and four dithered formats, the finish kernel in those with and without the sums.  And the 43 untrimmed
    instantiations beside them: the same figures without the product's multiply."""
    out = str(tmp_path / "io.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "io.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @(.*?)^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        if "_trim_" in m.group(1):
            body = m.group(2)
            found[m.group(1)] = (int(m.group(3)), int(m.group(4)), int(m.group(5)), body.count("v_fma_f64"), body.count("v_mul_f64"), body.count("atomic"),
                                 body.count("scratch_"))
    kinds = {k: sum(1 for n in found if k in n) for k in ("wave_encode4_rows_trim_kernel", "finish_master_trim_kernel", "wave_encode4_trim_kernel", "wave_encode_trim_tail_kernel")}
    assert kinds == {"wave_encode4_rows_trim_kernel": 10, "finish_master_trim_kernel": 20, "wave_encode4_trim_kernel": 10, "wave_encode_trim_tail_kernel": 10}, kinds
    for name, (vgprs, scratch, lds, fma, mul, atomic, scratch_ops) in found.items():
        assert scratch == 0 and scratch_ops == 0 and lds == 0 and fma == 0 and atomic == 0 and mul >= 1 and vgprs <= 128, (name, vgprs, scratch, lds, fma, mul, atomic)
    # The plain and the dithered kernels, which the same three launchers start with the trim off: the same figures, and the only v_mul_f64
    # are the quantiser's scale -- one per LPCM sample a thread encodes (4 per group, 8 in the finish's two sides, 1 in the tail), none
    # for the IEEE formats.  A multiply by a gain of 1.0 would show here.
    per_thread = {"wave_encode4_rows_kernel": 4, "wave_encode4_rows_dither_kernel": 4, "finish_master_kernel": 8, "finish_master_dither_kernel": 8,
                  "wave_encode4_kernel": 4, "wave_encode4_dither_kernel": 4, "wave_encode_dither_tail_kernel": 1}
    untrimmed = {k: 0 for k in per_thread}
    for m in re.finditer(r"^(_Z\d+([a-z0-9_]+)ILi(\d+)E\w+):\s*; @(.*?)^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        name, kind, fmt, body = m.group(1), m.group(2), int(m.group(3)), m.group(4)
        if kind not in per_thread:
            continue
        untrimmed[kind] += 1
        figures = (int(m.group(5)), int(m.group(6)), int(m.group(7)), body.count("v_fma_f64"), body.count("atomic"), body.count("scratch_"))
        assert figures[1:] == (0, 0, 0, 0, 0) and figures[0] <= 128, (name, figures)
        assert body.count("v_mul_f64") == (per_thread[kind] if fmt <= 3 else 0), (name, body.count("v_mul_f64"))
    # the plain kernels in five formats (IEEE64's rows are a copy, its bytes the one-sample kernel's; the bulk kernel's IEEE64 instantiation
    # is never launched), the dithered ones in four, the finish in six and four with and without the sums
    assert untrimmed == {"wave_encode4_rows_kernel": 5, "wave_encode4_rows_dither_kernel": 4, "finish_master_kernel": 12, "finish_master_dither_kernel": 8,
                         "wave_encode4_kernel": 6, "wave_encode4_dither_kernel": 4, "wave_encode_dither_tail_kernel": 4}, untrimmed
