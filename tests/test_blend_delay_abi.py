"""The delayed blend entry points at the drop-in boundary, without a GPU: the new prototypes compile as pedantic C99 and link by their
plain names, libgdg.so exports them, header and exports stay set-equal, the header carries the limit and the normative text, every layer
knows the calls, and the compiler's own summary shows that the two new kernels use no scratch, no LDS, no atomics and no fused
multiply-add."""
import ctypes
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
NEW = ["gdg_batch_set_blends_delayed", "gdg_batch_blend_max_delay", "gdg_blend_rows_delayed", "gdg_blend_rows_delayed_device", "gdg_blend_delays_from_align"]

C_PROBE = r"""
#include <stdio.h>
#include <string.h>
#include "gdg.h"
int main(void) {
    const int first[2] = { 0, 2 }, channel[2] = { 0, 1 }, delay[2] = { 0, 1 }, ref[2] = { -1, 0 };
    const double weight[2] = { 1.0, -1.0 }, gain[1] = { 1.0 };
    double a[2] = { 1.0, 2.0 }, b[2] = { 3.0, 4.0 }, o[2] = { 0.0, 0.0 };
    const double *rows[2];
    double *out[1];
    gdg_block_align rec[2];
    int d[2] = { 9, 9 }, s[2] = { 9, 9 }, rc;
    rows[0] = a; rows[1] = b; out[0] = o;
    memset(rec, 0, sizeof rec);
    rec[1].corr = -3.0; rec[1].ref_sq = 4.0; rec[1].sq_at_lag = 4.0; rec[1].lag = 37;
    printf("%d %d %d %d\n", gdg_batch_set_blends_delayed(NULL, 1, first, channel, weight, delay, gain), gdg_batch_blend_max_delay(NULL),
           gdg_blend_rows_delayed(NULL, rows, 2, 2, 1, first, channel, weight, delay, NULL, out),
           gdg_blend_rows_delayed_device(NULL, a, 2, 2, 2, 1, first, channel, weight, delay, NULL, GDG_BLEND_MAX_DELAY, o, 2));
    rc = gdg_blend_delays_from_align(rec, 2, 1, ref, 0.5, 1, first, channel, d, s);
    printf("%d %d %d %d %d\n", rc, d[0], d[1], s[0], s[1]);
    printf("%d\n", GDG_BLEND_MAX_DELAY);
    return 0;
}
"""


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_the_prototypes_are_pedantic_c99_and_link_from_c(pkg, tmp_path):
    src = tmp_path / "blend_delay_probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "blend_delay_probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    inv = pkg.GDG_ERR_INVALID
    assert [int(v) for v in lines[0].split()] == [inv, 0, inv, inv]                 # no context: refused, nothing touched; no delay in force
    assert [int(v) for v in lines[1].split()] == [0, 37, 0, 1, -1]                  # the planner needs no context: port 1 lies 37 late, inverted
    assert lines[2] == "4096"


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
    for name in ("batch_set_blends", "batch_blend_max_delay", "blend_rows_delayed", "blend_rows_delayed_device"):
        assert callable(getattr(pkg.Context, name)), name
    assert callable(pkg.blend_delays_from_align) and pkg.BLEND_MAX_DELAY == 4096
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = f.read()
    assert re.search(r"^int gdg_batch_set_blends_delayed\(gdg_ctx \*ctx, int n_blends, const int \*first, const int \*channel, const double \*weight, const int \*delay,$", header, re.M)
    assert re.search(r"^int gdg_batch_blend_max_delay\(const gdg_ctx \*ctx\);", header, re.M)
    assert re.search(r"^#define GDG_BLEND_MAX_DELAY 4096$", header, re.M)
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("x_k[i] = x[c_k][i - d_k] for i >= d_k", "x_k[i] = +0.0 for i < d_k", "the last d_k samples of a delayed term are never written",
                   "Stateless per sample while every delay is 0", "give the first difference of the row", "s[0] = x[0] - (+0.0)",
                   "history[r][GDG_BLEND_MAX_DELAY - 1] is sample -1", "Read, never written", "the lower median", "delay_k = max_j lag_j - lag_k",
                   "is not in the version-1 checkpoint container", "return GDG_ERR_UNSUPPORTED and write nothing", "counted by stat_batch_device_kib"):
        assert phrase in flat, phrase
    with open(os.path.join(CSRC, "blend.h")) as f:
        plain = f.read()
    assert "hip/hip_runtime" not in plain and "BLEND_DELAY" in plain and "gdg_blend_plan_delays" in plain
    with open(os.path.join(CSRC, "blend_kernels.h")) as f:
        kernels = f.read()
    assert "blend_delayed_kernel" in kernels and "blend_history_save_kernel" in kernels and "gdg_launch_blend(" in kernels
    base = os.path.dirname(os.path.dirname(pkg.LIB_PATH))
    with open(os.path.join(base, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    assert re.search(r"^func \(this \*Context\) BatchSetBlendsDelayed\(blends \[\]\[\]BlendTerm, delay \[\]\[\]int, gain \[\]float64\) error", go, re.M)
    assert re.search(r"^func \(this \*Context\) BatchBlendMaxDelay\(\) int", go, re.M)
    assert re.search(r"^func \(this \*Context\) BlendRowsDelayed\(", go, re.M) and re.search(r"^func \(this \*Context\) BlendRowsDelayedDevice\(", go, re.M)
    assert re.search(r"^func BlendDelaysFromAlign\(", go, re.M)
    for call in ("C.gdg_batch_set_blends_delayed(", "C.gdg_batch_blend_max_delay(", "C.gdg_blend_rows_delayed(", "C.gdg_blend_rows_delayed_device(", "C.gdg_blend_delays_from_align("):
        assert call in go, call
    from go_dsp_guitar_amd import host
    assert callable(host.Engine.render_aligned) and host.lib().gdgh_engine_set_batch_blends_delayed is not None
    with open(os.path.join(base, "host", "gdg_host.hpp")) as f:
        assert "const std::vector<std::vector<int>> &delay = {}" in f.read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "probes", "batch_blend_delay.py"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_delayed_kernels_use_no_scratch_no_lds_and_no_atomics(tmp_path):
    """Both instantiations of blend_delayed_kernel and of blend_history_save_kernel (16-byte and 8-byte lanes), from the compiler's resource
    summary: no scratch, no LDS, no atomics, no fused multiply-add of doubles; the sum's products and adds are v_mul_f64 and v_add_f64 of
    their own, its term table -- with the delays -- comes through scalar loads, and the 16-byte form keeps a 16-byte store."""
    out = str(tmp_path / "io.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "io.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @(.*?)^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        if "blend_delayed_kernel" in m.group(1) or "blend_history_save_kernel" in m.group(1):
            body = m.group(2)
            found[m.group(1)] = dict(vgprs=int(m.group(3)), scratch=int(m.group(4)), lds=int(m.group(5)), fma=body.count("v_fma_f64"), mul=body.count("v_mul_f64"),
                                     add=body.count("v_add_f64"), atomic=body.count("atomic"), scratch_ops=body.count("scratch_"), ds_ops=body.count("ds_"),
                                     s_loads=body.count("s_load_dword"), wide_stores=body.count("global_store_dwordx4"))
    sums = {n: f for n, f in found.items() if "blend_delayed_kernel" in n}
    saves = {n: f for n, f in found.items() if "blend_history_save_kernel" in n}
    assert len(sums) == 2 and len(saves) == 2, sorted(found)
    for name, f in found.items():
        assert f["scratch"] == 0 and f["scratch_ops"] == 0 and f["lds"] == 0 and f["ds_ops"] == 0 and f["fma"] == 0 and f["atomic"] == 0, (name, f)
    for name, f in sums.items():
        assert f["mul"] >= 1 and f["add"] >= 1 and f["s_loads"] >= 4 and f["vgprs"] <= 128, (name, f)
    for name, f in saves.items():
        assert f["mul"] == 0 and f["add"] == 0, (name, f)
    assert sorted(f["wide_stores"] > 0 for f in sums.values()) == [False, True] and sorted(f["wide_stores"] > 0 for f in saves.values()) == [False, True]
