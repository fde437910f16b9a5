"""CPU side of the checkpoint entry points (gdg_batch_stream_checkpoint_size / _checkpoint / _resume / _resume_shard, gdg_state_verify):
declared in include/gdg.h as plain C99, exported by libgdg.so, known to the Python layer, the Go binding and the C++ twin; and the
plain-Python restatement of the container's digest (the yardstick of tests/test_gpu_checkpoint.py) against vectors made by hand."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
NAMES = ["gdg_batch_stream_checkpoint_size", "gdg_batch_stream_checkpoint", "gdg_batch_stream_resume", "gdg_batch_stream_resume_shard",
         "gdg_state_verify"]

C_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "gdg.h"
int main(void) {
    gdg_ctx *ctx = NULL;
    gdg_batch_input in[2] = { { NULL, 0, 0, 0, 0, 0 }, { NULL, 0, 0, 0, 0, 0 } };
    gdg_batch_options opt = { 48000, GDG_FMT_LPCM24, 0, 0, 0 };
    size_t bytes = 0, written = 0, done = 0;
    unsigned char blob[64] = { 0 };
    int r[5];
    r[0] = gdg_batch_stream_checkpoint_size(ctx, &bytes);
    r[1] = gdg_batch_stream_checkpoint(ctx, blob, sizeof(blob), &written);
    r[2] = gdg_batch_stream_resume(ctx, in, 2, &opt, blob, sizeof(blob), &done);
    r[3] = gdg_batch_stream_resume_shard(ctx, in, 2, &opt, 8192, 1, blob, sizeof(blob), &done);
    r[4] = gdg_state_verify(ctx, blob, sizeof(blob));
    printf("%d %d %d %d %d\n", r[0], r[1], r[2], r[3], r[4]);
    return 0;
}
"""

M64 = (1 << 64) - 1
K, M0, M1 = 0x9e3779b97f4a7c15, 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53


def digest(payload):
    """include/gdg.h's digest of a container's payload, restated: granule g = the little-endian 64-bit words a, b;
    u = t ^ (t >> 32), t = (a + (g + 1) K) M0;  v = s ^ (s >> 29), s = (b ^ u) M1;  S0 = sum u, S1 = xor v (mod 2^64);
    D0 = fmix(S0 + K + n), D1 = fmix(S1 ^ D0) with murmur3's 64-bit finalizer.  -> 16 bytes."""
    assert len(payload) % 16 == 0
    n = len(payload) // 16
    s0 = s1 = 0
    for g in range(n):
        a = int.from_bytes(payload[16 * g:16 * g + 8], "little")
        b = int.from_bytes(payload[16 * g + 8:16 * g + 16], "little")
        t = ((a + (g + 1) * K) * M0) & M64
        u = t ^ (t >> 32)
        s = ((b ^ u) * M1) & M64
        v = s ^ (s >> 29)
        s0 = (s0 + u) & M64
        s1 ^= v

    def fmix(x):
        x ^= x >> 33
        x = (x * M0) & M64
        x ^= x >> 33
        x = (x * M1) & M64
        return x ^ (x >> 33)
    d0 = fmix((s0 + K + n) & M64)
    d1 = fmix(s1 ^ d0)
    return d0.to_bytes(8, "little") + d1.to_bytes(8, "little")


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def _header():
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        return f.read()


def test_the_prototypes_are_in_the_header_and_say_what_the_digest_is():
    text = _header()
    for name in NAMES:
        assert re.search(r"^int %s\(gdg_ctx \*ctx" % name, text, re.M), name
    assert "GDGCKPT" in text and "INTEGRITY ONLY" in text
    for const in ("0x9e3779b97f4a7c15", "0xff51afd7ed558ccd", "0xc4ceb9fe1a85ec53"):
        assert const in text, "the header states the digest's constants"
    # the sentence that sent the reader away now names what the state blob still leaves out, and where it went
    assert "meters, the metronome, batch-run buffers" not in text


def test_the_library_exports_them_and_the_python_layer_knows_them(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert name in exported, name
        assert name in pkg.ABI_SYMBOLS, name
        assert getattr(pkg.lib(), name).argtypes is not None
    for meth in ("batch_stream_checkpoint", "batch_stream_resume", "batch_stream_resume_shard", "state_verify"):
        assert callable(getattr(pkg.Context, meth))


def test_the_header_is_c99_and_the_calls_link(pkg, tmp_path):
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "gdg.h")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = tmp_path / "checkpoint_probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "checkpoint_probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert [int(v) for v in r.stdout.split()] == [pkg.GDG_ERR_INVALID] * 5


def test_the_go_binding_and_the_cpp_twin_declare_their_counterparts(pkg):
    here = os.path.dirname(pkg.LIB_PATH)
    base = os.path.dirname(here)
    with open(os.path.join(base, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    for fn, c in (("BatchStreamCheckpoint", "gdg_batch_stream_checkpoint"), ("BatchStreamResume", "gdg_batch_stream_resume"),
                  ("BatchStreamResumeShard", "gdg_batch_stream_resume_shard"), ("StateVerify", "gdg_state_verify")):
        assert re.search(r"^func \(this \*Context\) %s\(" % fn, go, re.M), fn
        assert "C.%s(" % c in go, c
    with open(os.path.join(base, "host", "gdg_host.hpp")) as f:
        hpp = f.read()
    with open(os.path.join(base, "host", "gdg_host.cpp")) as f:
        cpp = f.read()
    for fn in ("BatchStreamCheckpoint", "BatchStreamResume", "BatchStreamShardedCheckpoint", "BatchStreamShardedResume"):
        assert re.search(r"Error %s\(" % fn, hpp), fn
        assert re.search(r"^Error Engine::%s\(" % fn, cpp, re.M), fn
    assert "gdg_batch_stream_resume_shard(" in cpp and "this engine has %d" in cpp      # another shard count is refused


def test_the_digest_restatement_on_hand_made_vectors(pkg):
    def fmix(x):
        x ^= x >> 33
        x = (x * M0) & M64
        x ^= x >> 33
        x = (x * M1) & M64
        return x ^ (x >> 33)
    # empty payload: no granule, S0 = S1 = 0, n = 0
    d0 = fmix(K)
    assert digest(b"") == d0.to_bytes(8, "little") + fmix(d0).to_bytes(8, "little")
    # one granule of zeros, worked by hand: a = b = 0, g = 0
    t = (K * M0) & M64
    u = t ^ (t >> 32)
    s = (u * M1) & M64
    v = s ^ (s >> 29)
    d0 = fmix((u + K + 1) & M64)
    assert digest(bytes(16)) == d0.to_bytes(8, "little") + fmix(v ^ d0).to_bytes(8, "little")
    # two granules and the same two swapped: order matters
    g0, g1 = bytes(range(16)), bytes(range(100, 116))
    assert digest(g0 + g1) != digest(g1 + g0)
    assert digest(g0 + g1)[:8] != digest(g1 + g0)[:8] and digest(g0 + g1)[8:] != digest(g1 + g0)[8:]
    # length matters (trailing zero granules), and so does every bit
    assert digest(g0) != digest(g0 + bytes(16))
    flipped = bytearray(g0 + g1)
    flipped[23] ^= 0x10
    assert digest(bytes(flipped)) != digest(g0 + g1)
    # the package's own restatement (for tools without a GPU) is the same function
    rng_bytes = bytes((i * 37 + 11) & 0xff for i in range(16 * 9))
    for p in (b"", bytes(16), g0 + g1, rng_bytes):
        assert pkg.checkpoint_digest(p) == digest(p)
