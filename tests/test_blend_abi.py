"""The blend entry points at the drop-in boundary, without a GPU: the new prototypes compile as pedantic C99 and link by their plain names,
libgdg.so exports them, header and exports stay set-equal, the header carries the limits and the normative text, every layer knows the
calls, and the compiler's own summary shows that the new kernel uses no scratch, no LDS, no atomics and no fused multiply-add."""
import ctypes
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
NEW = ["gdg_batch_set_blends", "gdg_batch_blends", "gdg_blend_rows", "gdg_blend_rows_device"]

C_PROBE = r"""
#include <stdio.h>
#include "gdg.h"
int main(void) {
    const int first[2] = { 0, 2 }, channel[2] = { 0, 1 };
    const double weight[2] = { 0.6, 0.4 }, gain[1] = { 1.0 };
    double a[2] = { 1.0, 2.0 }, b[2] = { 3.0, 4.0 }, o[2] = { 0.0, 0.0 };
    const double *rows[2];
    double *out[1];
    rows[0] = a; rows[1] = b; out[0] = o;
    printf("%d %d %d %d\n", gdg_batch_set_blends(NULL, 1, first, channel, weight, gain), gdg_batch_blends(NULL),
           gdg_blend_rows(NULL, rows, 2, 2, 1, first, channel, weight, out), gdg_blend_rows_device(NULL, a, 2, 2, 2, 1, first, channel, weight, o, 2));
    printf("%d %d\n", GDG_BLEND_MAX_TERMS, GDG_BLEND_MAX_BLENDS);
    return 0;
}
"""


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_the_prototypes_are_pedantic_c99_and_link_from_c(pkg, tmp_path):
    src = tmp_path / "blend_probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "blend_probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    inv = pkg.GDG_ERR_INVALID
    assert [int(v) for v in lines[0].split()] == [inv, 0, inv, inv]                 # no context: refused, nothing touched; no blend in force
    assert lines[1] == "32 1024"


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
    for name in ("batch_set_blends", "batch_blends", "blend_rows", "blend_rows_device"):
        assert callable(getattr(pkg.Context, name)), name
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = f.read()
    assert re.search(r"^int gdg_batch_set_blends\(gdg_ctx \*ctx, int n_blends, const int \*first, const int \*channel, const double \*weight, const double \*gain\);", header, re.M)
    assert re.search(r"^int gdg_batch_blends\(const gdg_ctx \*ctx\);", header, re.M)
    assert re.search(r"^#define GDG_BLEND_MAX_TERMS 32$", header, re.M) and re.search(r"^#define GDG_BLEND_MAX_BLENDS 1024$", header, re.M)
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("ONE rounded IEEE-754 double multiply", "in term order", "never contracted into a fused multiply-add and never reassociated",
                   "give 0.6000000000000001; the same terms in reverse order give 0.6", "port N + 3 + b", "port_base + N + 3 + b", "0 inf is NaN", "the sign and the payload of a NaN the arithmetic produces are not",
                   "before the trim, before the spatializer", "stat_batch_device_kib is unchanged", "GDG_ERR_UNSUPPORTED while blends are in force"):
        assert phrase in flat, phrase
    with open(os.path.join(CSRC, "blend.h")) as f:
        plain = f.read()
    assert "hip/hip_runtime" not in plain and "gdg_blend_check" in plain                # a stand-alone program can drive it
    base = os.path.dirname(os.path.dirname(pkg.LIB_PATH))
    with open(os.path.join(base, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    assert re.search(r"^func \(this \*Context\) BatchSetBlends\(blends \[\]\[\]BlendTerm, gain \[\]float64\) error", go, re.M)
    assert re.search(r"^func \(this \*Context\) BlendRows\(rows \[\]\[\]float64, blends \[\]\[\]BlendTerm\) \(\[\]\[\]float64, error\)", go, re.M)
    assert re.search(r"^func \(this \*Context\) BlendRowsDevice\(", go, re.M)
    for call in ("C.gdg_batch_set_blends(", "C.gdg_batch_blends(", "C.gdg_blend_rows(", "C.gdg_blend_rows_device("):
        assert call in go, call
    from go_dsp_guitar_amd import host
    assert callable(host.Engine._set_blends) and host.lib().gdgh_engine_set_batch_blends is not None
    with open(os.path.join(base, "host", "gdg_host.hpp")) as f:
        assert "Error SetBatchBlends(const std::vector<std::vector<std::pair<int, double>>> &blends" in f.read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "probes", "batch_blend.py"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_blend_kernel_uses_no_scratch_and_no_lds(tmp_path):
    """Both instantiations of blend_rows_kernel (16-byte and 8-byte lanes), from the compiler's resource summary: no scratch, no LDS, no atomics,
    every product a v_mul_f64 and every add a v_add_f64 of its own -- no fused multiply-add of doubles -- and the term table through scalar
    loads."""
    out = str(tmp_path / "io.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "io.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @(.*?)^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        if "blend_rows_kernel" in m.group(1):
            body = m.group(2)
            found[m.group(1)] = (int(m.group(3)), int(m.group(4)), int(m.group(5)), body.count("v_fma_f64"), body.count("v_mul_f64"), body.count("v_add_f64"),
                                 body.count("atomic"), body.count("scratch_"), body.count("ds_"), body.count("s_load_dword"))
    assert len(found) == 2, sorted(found)
    for name, (vgprs, scratch, lds, fma, mul, add, atomic, scratch_ops, ds_ops, s_loads) in found.items():
        assert scratch == 0 and scratch_ops == 0 and lds == 0 and ds_ops == 0 and fma == 0 and atomic == 0, (name, scratch, lds, fma, atomic)
        assert mul >= 1 and add >= 1 and s_loads >= 3 and vgprs <= 64, (name, vgprs, mul, add, s_loads)
