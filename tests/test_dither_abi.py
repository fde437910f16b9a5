"""The dither entry points at the drop-in boundary, without a GPU: the new prototypes compile as pedantic C99 and link by their plain names,
libgdg.so exports them, header and exports stay set-equal, and every layer knows the calls."""
import ctypes
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
NEW = ["gdg_batch_set_dither", "gdg_batch_dither_seek", "gdg_wave_encode_dither", "gdg_wave_encode_dither_device"]

C_PROBE = r"""
#include <stdio.h>
#include "gdg.h"
int main(void) {
    double x[4] = { 0.0, 0.25, -0.5, 1.0 };
    unsigned char out[16];
    const uint64_t seed = 0xdeadbeefcafef00dULL, first = 0x10000000001ULL;
    const uint32_t port = 0xfffffffdU;
    printf("%d %d %d %d\n", gdg_batch_set_dither(NULL, 1, seed, 0), gdg_batch_dither_seek(NULL, first),
           gdg_wave_encode_dither(NULL, GDG_FMT_LPCM16, x, 4, 1, seed, port, first, out),
           gdg_wave_encode_dither_device(NULL, GDG_FMT_LPCM24, x, 4, 1, seed, port, first, out));
    return 0;
}
"""


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_the_prototypes_are_pedantic_c99_and_link_from_c(pkg, tmp_path):
    src = tmp_path / "dither_probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "dither_probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert [int(v) for v in r.stdout.split()] == [pkg.GDG_ERR_INVALID] * 4          # no context: refused, nothing touched


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
    for name in ("batch_set_dither", "batch_dither_seek", "wave_encode_dither", "wave_encode_dither_device"):
        assert callable(getattr(pkg.Context, name)), name
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = f.read()
    assert re.search(r"^int gdg_batch_set_dither\(gdg_ctx \*ctx, int mode, uint64_t seed, uint32_t port_base\);", header, re.M)
    assert re.search(r"^int gdg_batch_dither_seek\(gdg_ctx \*ctx, uint64_t sample_index\);", header, re.M)
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("master left 0xfffffffd", "part of no blob", "0xdf9545e13007448a", "No noise shaping"):
        assert phrase in flat, phrase
    base = os.path.dirname(os.path.dirname(pkg.LIB_PATH))
    with open(os.path.join(base, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    assert re.search(r"^func \(this \*Context\) BatchSetDither\(mode int, seed uint64, portBase uint32\) error", go, re.M) and "C.gdg_batch_set_dither(" in go
    assert re.search(r"^func \(this \*Context\) BatchDitherSeek\(sampleIndex uint64\) error", go, re.M) and "C.gdg_batch_dither_seek(" in go
    assert "C.gdg_wave_encode_dither(" in go
