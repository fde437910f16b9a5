"""CPU side of the channel-state entry points (gdg_state_*): a C program that calls every one of them compiles as plain C99 against
include/gdg.h and links against libgdg.so by the plain names.  Without a GPU there is no context, and every call on a NULL one is refused."""
import os
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT

C_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "gdg.h"
int main(void) {
    gdg_ctx *ctx = NULL;
    int channels[2] = { 5, 2 };
    size_t bytes = 0, written = 0;
    unsigned char blob[64];
    int r[5];
    r[0] = gdg_state_size(ctx, channels, 2, &bytes);
    r[1] = gdg_state_save(ctx, NULL, 0, blob, sizeof(blob), &written);
    r[2] = gdg_state_save_device(ctx, channels, 2, blob, sizeof(blob), &written);
    r[3] = gdg_state_load(ctx, channels, 2, blob, sizeof(blob));
    r[4] = gdg_state_load_device(ctx, NULL, 0, blob, sizeof(blob));
    printf("%d %d %d %d %d\n", r[0], r[1], r[2], r[3], r[4]);
    return 0;
}
"""


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_state_prototypes_compile_as_c_and_link(pkg, tmp_path):
    src = tmp_path / "state_probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "state_probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert [int(v) for v in r.stdout.split()] == [pkg.GDG_ERR_INVALID] * 5


def test_the_python_layer_knows_the_entry_points(pkg):
    for name in ("gdg_state_size", "gdg_state_save", "gdg_state_save_device", "gdg_state_load", "gdg_state_load_device"):
        assert name in pkg.ABI_SYMBOLS
        assert getattr(pkg.lib(), name).argtypes is not None
    for meth in ("state_size", "save_state", "load_state", "save_state_device", "load_state_device"):
        assert callable(getattr(pkg.Context, meth))
