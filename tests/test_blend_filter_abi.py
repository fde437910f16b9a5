"""The filtered blend entry points at the drop-in boundary, without a GPU: the new prototypes compile as pedantic C99 and link by their
plain names, libgdg.so exports them, header and exports stay set-equal, the header carries the limit and the normative text, and the
compiler's own summary shows that both instantiations of the filtered kernel use no scratch, no atomics and no fused multiply-add, and the
LDS that DESIGN.md 4.12f states."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
NEW = ["gdg_batch_set_blends_filtered", "gdg_batch_blend_max_reach", "gdg_blend_rows_filtered", "gdg_blend_rows_filtered_device", "gdg_blend_fraction_taps",
       "gdg_blend_fractions_from_fit"]

C_PROBE = r"""
#include <stdio.h>
#include <string.h>
#include "gdg.h"
int main(void) {
    const int first[2] = { 0, 1 }, channel[1] = { 0 }, delay[1] = { 0 }, tap_first[2] = { 0, 2 };
    const double weight[1] = { 1.0 }, tap[2] = { 1.0, -1.0 }, gain[1] = { 1.0 };
    double a[2] = { 1.0, 2.0 }, o[2] = { 0.0, 0.0 }, h[4] = { 9.0, 9.0, 9.0, 9.0 };
    const double *rows[1];
    double *out[1];
    gdg_block_fit rec[1];
    int step[1] = { 9 }, rc;
    rows[0] = a; out[0] = o;
    memset(rec, 0, sizeof rec);
    rec[0].terms = 3; rec[0].tt = 1.0; rec[0].tx[0] = 1.0; rec[0].tx[1] = 2.0; rec[0].tx[2] = 5.0; rec[0].xx[0] = 1.0; rec[0].xx[2] = 1.0; rec[0].xx[5] = 4.0;
    printf("%d %d %d %d\n", gdg_batch_set_blends_filtered(NULL, 1, first, channel, weight, delay, tap_first, tap, gain), gdg_batch_blend_max_reach(NULL),
           gdg_blend_rows_filtered(NULL, rows, 1, 2, 1, first, channel, weight, delay, tap_first, tap, NULL, out),
           gdg_blend_rows_filtered_device(NULL, a, 2, 1, 2, 1, first, channel, weight, delay, tap_first, tap, NULL, GDG_BLEND_MAX_DELAY, o, 2));
    rc = gdg_blend_fraction_taps(4, 0.0, h);
    printf("%d %g %g %g %g\n", rc, h[0], h[1], h[2], h[3]);
    rc = gdg_blend_fractions_from_fit(rec, 1, 1, 2, step);
    printf("%d %d\n", rc, step[0]);
    printf("%d %d\n", GDG_BLEND_MAX_TAPS, gdg_blend_fraction_taps(3, 0.5, h));
    return 0;
}
"""


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_the_prototypes_are_pedantic_c99_and_link_from_c(pkg, tmp_path):
    src = tmp_path / "blend_filter_probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "blend_filter_probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    inv = pkg.GDG_ERR_INVALID
    assert [int(v) for v in lines[0].split()] == [inv, 0, inv, inv]                 # no context: refused, nothing touched; nothing in force
    assert lines[1].split() == ["0", "0", "1", "0", "0"]                            # the planner needs no context: the impulse at T/2 - 1
    assert [int(v) for v in lines[2].split()] == [0, 1]                             # scores 1, 2, 2.5: the candidate at +1/2
    assert [int(v) for v in lines[3].split()] == [64, inv]


def test_the_symbols_are_exported_and_header_and_exports_stay_set_equal(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdg.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(gdg_[a-z_0-9]+)\s*\(", header))
    for name in NEW:
        assert name in exported and name in declared and name in pkg.ABI_SYMBOLS, name
        assert getattr(pkg.lib(), name).argtypes is not None
    assert {n for n in exported if n.startswith("gdg_")} == declared == set(pkg.ABI_SYMBOLS)


def test_every_layer_knows_the_calls(pkg):
    for name in ("batch_set_blends", "batch_blend_max_reach", "blend_rows_filtered", "blend_rows_filtered_device"):
        assert callable(getattr(pkg.Context, name)), name
    assert callable(pkg.blend_fraction_taps) and callable(pkg.blend_fractions_from_fit) and pkg.BLEND_MAX_TAPS == 64
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = f.read()
    assert re.search(r"^int gdg_batch_set_blends_filtered\(gdg_ctx \*ctx, int n_blends, const int \*first, const int \*channel, const double \*weight, const int \*delay,$", header, re.M)
    assert re.search(r"^int gdg_batch_blend_max_reach\(const gdg_ctx \*ctx\);", header, re.M)
    assert re.search(r"^int gdg_blend_fraction_taps\(int n_taps, double fraction, double \*tap\);", header, re.M)
    assert re.search(r"^int gdg_blend_fractions_from_fit\(const gdg_block_fit \*records, int n_fits, size_t blocks, int steps, int \*step\);", header, re.M)
    assert re.search(r"^#define GDG_BLEND_MAX_TAPS 64$", header, re.M)
    assert header.index(" * DELAYS:") < header.index(" * FILTERS:") < header.index("#define GDG_BLEND_MAX_TERMS")
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("T_k == 0: x_k[i] = x[c_k][i - d_k]", "f = h_k[0] x[c_k][i - d_k]", "f = f + (h_k[t] x[c_k][i - d_k - t])", "ascending t",
                   "d_k + max(T_k, 1) - 1 <= GDG_BLEND_MAX_DELAY", "d = 0, T = 2, h = {1, -1} and w = 1 gives s[0] = x[0] and s[i] = x[i] - x[i - 1]",
                   "a NaN at x[c][j] reaches i = j + d .. j + d + T - 1", "tap_first == NULL: the call IS gdg_batch_set_blends_delayed",
                   "return GDG_ERR_UNSUPPORTED while gdg_batch_blend_max_reach > 0", "the exact unit impulse at T/2 - 1", "the earlier entry wins a tie",
                   "zeroed by the first slice of a job", "counted by stat_batch_device_kib"):
        assert phrase in flat, phrase
    with open(os.path.join(CSRC, "blend.h")) as f:
        plain = f.read()
    assert "hip/hip_runtime" not in plain and "gdg_blend_check_taps" in plain and "gdg_blend_plan_fractions" in plain
    with open(os.path.join(CSRC, "blend_kernels.h")) as f:
        kernels = f.read()
    assert "blend_filtered_kernel" in kernels and "gdg_launch_blend(" in kernels


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_filtered_kernel_uses_no_scratch_no_atomics_and_the_lds_the_design_states(tmp_path):
    """Both instantiations of blend_filtered_kernel (16-byte and 8-byte lanes), from the compiler's resource summary: no scratch, no atomics,
    no fused multiply-add of doubles; products and adds are v_mul_f64 and v_add_f64 of their own; the table -- with tap_first and the taps
    -- comes through scalar loads; the 16-byte form keeps a 16-byte store; and the LDS is the two windows DESIGN.md 4.12f states."""
    out = str(tmp_path / "io.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "io.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @(.*?)^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        if "blend_filtered_kernel" in m.group(1):
            body = m.group(2)
            found[m.group(1)] = dict(vgprs=int(m.group(3)), scratch=int(m.group(4)), lds=int(m.group(5)), fma=body.count("v_fma_f64"), mul=body.count("v_mul_f64"),
                                     add=body.count("v_add_f64"), atomic=body.count("atomic"), scratch_ops=body.count("scratch_"), s_loads=body.count("s_load_dword"),
                                     wide_stores=body.count("global_store_dwordx4"), barriers=body.count("s_barrier"))
    assert len(found) == 2, sorted(found)
    for name, f in found.items():
        assert f["scratch"] == 0 and f["scratch_ops"] == 0 and f["fma"] == 0 and f["atomic"] == 0, (name, f)
        assert f["mul"] >= 2 and f["add"] >= 2 and f["s_loads"] >= 6 and f["barriers"] >= 2 and f["vgprs"] <= 128, (name, f)
    assert sorted(f["wide_stores"] > 0 for f in found.values()) == [False, True]
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    section = design[design.index("4.12f"):]
    stated = {int(v) for v in re.findall(r"\| LDS \(bytes\) \| (\d+) \| (\d+) \|", section)[0]}
    assert stated == {f["lds"] for f in found.values()} == {2 * (512 + 64) * 8, 2 * (256 + 64) * 8}, (stated, found)
