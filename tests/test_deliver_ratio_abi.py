"""The ratio stage's place in the C-ABI, without a GPU: exports equal prototypes, every layer knows the calls, the pure-arithmetic calls answer
without a context, what can be refused without a device is refused, and the compiler's resource summary: the new kernels use no scratch and
deliver_rows_kernel<2> and <4> keep the registers and LDS they had."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
CSRC = os.path.join(entry.PKG_DIR, "csrc")
NEW = ["gdg_batch_set_out_ratio", "gdg_batch_out_ratio", "gdg_batch_out_samples", "gdg_batch_out_ratio_latency", "gdg_out_ratio_taps",
       "gdg_out_ratio_rows", "gdg_out_ratio_rows_device"]


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
        assert getattr(pkg.lib(), name) is not None
    assert {n for n in exported if n.startswith("gdg_") and ("out_ratio" in n or "out_samples" in n)} == set(NEW)
    for method in ("batch_set_delivery_ratio", "batch_delivery_ratio", "batch_delivery_samples", "deliver_rows_ratio", "deliver_rows_ratio_device", "deliver_ratio_taps",
                   "batch_delivery_ratio_latency"):
        assert callable(getattr(pkg.Context, method)), method
    with open(os.path.join(entry.PKG_DIR, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    for name in NEW:
        assert "C.%s(" % name in go, name
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("T = 2 ceil(32 max(1, M / L))", "fc = 0.5 / max(L, M)", "beta = 10", "tap[p][t] = g[p + t L]", "b = floor(n M / L) and p = (n M) mod L", "in ascending order",
                   "ceil(s0 L / M) <= n < ceil(s1 L / M)", "gdg_batch_delivery_latency(R) + R T / 2", "y[n] = g[n M] while n M < L T", "silence gives exactly +0.0",
                   "ORDER: factor, ratio, then the trim or blend gain", "an unreduced pair is refused, naming the reduced one"):
        assert phrase in flat, phrase
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert re.search(r"^io\.o:.*deliver_ratio_kernels\.h", f.read(), re.M)


def test_arithmetic_without_a_context_and_null_contexts(pkg):
    lib = pkg.lib()
    assert pkg.batch_delivery_samples(4, 147, 160, 0, 3 * 8192) == 5645 and pkg.batch_delivery_ratio_latency(4, 147, 160) == 217
    assert pkg.deliver_ratio_taps(147, 160).shape == (147, 70) and pkg.deliver_ratio_taps(160, 147).shape == (160, 64)
    up, down = pkg.C.c_int(7), pkg.C.c_int(7)
    assert lib.gdg_batch_out_ratio(None, pkg.C.byref(up), pkg.C.byref(down)) == pkg.GDG_ERR_INVALID and (up.value, down.value) == (1, 1)
    assert lib.gdg_batch_set_out_ratio(None, 4, 147, 160) == pkg.GDG_ERR_INVALID
    x = np.zeros(8)
    assert lib.gdg_out_ratio_rows(None, x.ctypes.data, 1, 8, 147, 160, 0, None, x.ctypes.data, 8) == pkg.GDG_ERR_INVALID
    assert lib.gdg_out_ratio_rows_device(None, None, 8, 1, 8, 147, 160, 0, None, None, 8) == pkg.GDG_ERR_INVALID


def test_refusals_on_a_context(pkg):
    """an unreduced ratio, one outside the limits, setting while a stream is open: these need a context, so a device; without one the context
    cannot be made (tests/test_gpu_deliver_ratio.py holds them on the GPU)."""
    if pkg.device_count() == 0:
        with pytest.raises(pkg.GdgError) as e:
            pkg.Context(1, 8192)
        assert e.value.code == pkg.GDG_ERR_NO_DEVICE
        return
    ctx = pkg.Context(1, 8192)
    for args, text in (((1, 294, 320), "delivery ratio 294/320 is not reduced; pass 147/160"), ((1, 1, 3), "delivery ratio 1/3"), ((3, 147, 160), "delivery factor 3")):
        with pytest.raises(pkg.GdgError, match=text):
            ctx.batch_set_delivery_ratio(*args)
    assert ctx.batch_delivery() == 1 and ctx.batch_delivery_ratio() == (1, 1)
    ctx.close()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_new_kernels_use_no_scratch_and_the_factor_s_keep_their_resources(tmp_path):
    """From the compiler's resource summary of io.hip: deliver_ratio_kernel and deliver_ratio_history_save_kernel (C linkage: plain names) use no
    scratch, the ratio kernel 640 doubles of LDS and few enough registers for eight waves per SIMD, as DESIGN.md 4.12j states; every product
    and add on its own; deliver_rows_kernel<2> and <4> keep 26 and 36 VGPRs and 4 704 and 9 440 bytes of LDS."""
    out = str(tmp_path / "io.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "io.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (\w*deliver\w+)\n.*?^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    part = design[design.index("### 4.12j"):]
    table = {n: (int(v), int(s), int(lds.replace(" ", ""))) for n, v, s, lds in re.findall(r"^\| `(deliver\w+)` \| (\d+) \| (\d+) \| ([\d ]+) \|", part, re.M)}
    assert found["deliver_ratio_kernel"] == table["deliver_ratio_kernel"] and found["deliver_ratio_kernel"][1:] == (0, 640 * 8) and found["deliver_ratio_kernel"][0] <= 64
    assert found["deliver_ratio_history_save_kernel"] == table["deliver_ratio_history_save_kernel"] and found["deliver_ratio_history_save_kernel"][1:] == (0, 0)
    rows = {n: f for n, f in found.items() if "deliver_rows_kernel" in n}
    assert len(rows) == 4
    for name, figures in rows.items():
        assert figures == ((26, 0, 4704) if "ILi2E" in name else (36, 0, 9440)), (name, figures)
    kernel = re.search(r"^deliver_ratio_kernel:.*?\.amdhsa_kernel", text, re.S | re.M).group(0)
    assert "v_fma_f64" not in kernel and "v_mul_f64" in kernel and "v_add_f64" in kernel
