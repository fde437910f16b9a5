"""The delivery's place in the C-ABI, without a GPU: exports equal prototypes, the header compiles as pedantic C99 with the new calls in use,
every layer knows them, the pure-arithmetic calls answer, and what can be refused without a device is refused."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import deliver_ref as ref

ROOT = entry.ROOT
NEW = ["gdg_batch_set_delivery", "gdg_batch_delivery", "gdg_batch_delivery_latency", "gdg_deliver_rows", "gdg_deliver_rows_device", "gdg_deliver_taps"]


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
        assert name in exported and name in pkg.ABI_SYMBOLS and re.search(r"^int %s\(" % name, header, re.M), name
        assert getattr(pkg.lib(), name) is not None
    assert {n for n in exported if n.startswith("gdg_") and "deliver" in n and "launch" not in n} == set(NEW)
    for method in ("batch_set_delivery", "batch_delivery", "deliver_rows", "deliver_rows_device", "batch_delivery_latency", "deliver_taps"):
        assert callable(getattr(pkg.Context, method)), method
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("A = 0.9440608762859234", "in ascending order", "no fused multiply-add, and the symmetric taps are not folded", "an impulse at sample 1 gives y[i] = A h[R i - 1]",
                   "silence gives exactly +0.0", "WHAT STAYS AT THE SESSION RATE", "(the step's first session sample) / R + i", "decimate, then the gain",
                   "the history is not in the version-1 container", "without the clip to [-1, 1]"):
        assert phrase in flat, phrase
    with open(os.path.join(entry.PKG_DIR, "csrc", "Makefile")) as f:
        make = f.read()
    assert re.search(r"^io\.o:.*deliver_kernels\.h.*deliver\.h", make, re.M) and re.search(r"^api_%\.o:.*deliver\.h", make, re.M)


def test_latency_taps_and_null_contexts(pkg):
    lib = pkg.lib()
    assert [pkg.batch_delivery_latency(f) for f in (1, 2, 4)] == [0, 38, 77]
    assert [pkg.batch_delivery_latency(f) for f in (0, 3, 8, -1)] == [0, 0, 0, 0]
    for factor in (2, 4):
        assert np.array_equal(pkg.deliver_taps(factor), ref.taps(factor))
        few = np.full(5, 9.0)
        assert lib.gdg_deliver_taps(factor, few.ctypes.data, 3) == ref.TAPS[factor]
        assert np.array_equal(few[:3], ref.taps(factor)[:3]) and (few[3:] == 9.0).all()      # never past the capacity
    assert pkg.deliver_taps(1).size == 0 and pkg.deliver_taps(3).size == 0
    assert (pkg.DELIVER_HISTORY, pkg.DELIVER_ATTENUATION) == (154, ref.A)
    assert lib.gdg_batch_set_delivery(None, 2) == pkg.GDG_ERR_INVALID and lib.gdg_batch_delivery(None) == 1
    x = np.zeros(8)
    assert lib.gdg_deliver_rows(None, x.ctypes.data, 1, 8, 2, None, x.ctypes.data) == pkg.GDG_ERR_INVALID
    assert lib.gdg_deliver_rows_device(None, None, 8, 1, 8, 2, None, None, 4) == pkg.GDG_ERR_INVALID


C_PROBE = r"""
#include <stdio.h>
#include "gdg.h"
/* what cgo does with the header: compile it as C, link the new symbols by their plain names */
int main(void) {
    double taps[155], few[2] = { 0.0, 0.0 }, out[2];
    int n2 = gdg_deliver_taps(2, taps, 155), n4 = gdg_deliver_taps(4, taps, 155), n1 = gdg_deliver_taps(1, taps, 155);
    int rc = gdg_batch_set_delivery(NULL, 4);
    int rows = gdg_deliver_rows(NULL, few, 1, 2, 2, NULL, out);
    int dev = gdg_deliver_rows_device(NULL, few, 2, 1, 2, 2, NULL, out, 1);
    printf("%d %d %d|%d %d %d|%d %d %d|%d\n", n2, n4, n1, gdg_batch_delivery_latency(1), gdg_batch_delivery_latency(2), gdg_batch_delivery_latency(4), rc, rows, dev,
           gdg_batch_delivery(NULL));
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
    assert r.stdout.strip() == "77 155 0|0 38 77|%d %d %d|1" % (inv, inv, inv)


def test_refusals_on_a_context(pkg):
    """factor 3, factor 0, a sample count that is no multiple of the factor, setting while a stream is open: these need a context, so a device;
    without one the context cannot be made (tests/test_gpu_deliver.py holds them on the GPU)."""
    if pkg.device_count() == 0:
        with pytest.raises(pkg.GdgError) as e:
            pkg.Context(1, 8192)
        assert e.value.code == pkg.GDG_ERR_NO_DEVICE
        return
    ctx = pkg.Context(1, 8192)
    for bad in (0, 3):
        with pytest.raises(pkg.GdgError, match="delivery factor %d" % bad):
            ctx.batch_set_delivery(bad)
    with pytest.raises(pkg.GdgError, match="multiple of the delivery factor 4"):
        ctx.deliver_rows(np.zeros(6), 4)
    assert ctx.batch_delivery() == 1
    ctx.close()
