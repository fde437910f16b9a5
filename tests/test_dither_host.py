"""The CPU side of the dithered encoders (gdg_batch_set_dither): csrc/dither.h -- hash, key, noise, quantiser, the row-to-port mapping, the
range check and the cursor -- compiled without HIP into a stand-alone program under AddressSanitizer and UBSan, held against the known
answers of include/gdg.h and against a table this file makes with the numpy restatement (tests/dither_ref.py).  What the kernels write
is tests/test_gpu_dither.py's business."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import dither_ref as ref

ROOT = entry.ROOT
FMTS = ["lpcm8", "lpcm16", "lpcm24", "lpcm32"]


@pytest.fixture(scope="module")
def dither_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dither") / "dither_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "go-dsp-guitar_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "dither_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_the_restatement_gives_the_known_answers():
    for seed, port, index, x, h, c16, c24 in ref.KNOWN:
        assert int(ref.hashes(seed, port, index, 1)[0]) == h
        assert int(ref.codes("lpcm16", [x], seed, port, index)[0]) == c16
        assert int(ref.codes("lpcm24", [x], seed, port, index)[0]) == c24
    for fmt in FMTS:                                          # bytes -> codes -> bytes
        x = np.random.default_rng(3).uniform(-1.2, 1.2, 257)
        assert np.array_equal(ref.decode_codes(fmt, ref.encode(fmt, x, 5, 6, 7)), ref.codes(fmt, x, 5, 6, 7))


def test_the_header_gives_the_known_answers_and_maps_ports(dither_check):
    r = subprocess.run([dither_check], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


@pytest.mark.parametrize("seed", [1, 2])
def test_the_header_equals_the_restatement_on_random_samples(dither_check, tmp_path, seed):
    """4000 seeded (seed, port, index, x): samples all over +-1.3, tiny ones, exact code boundaries of every format and neighbours of the
    half-code points; ports among the fixed ids; indices around 2^32 and up to 2^64 - 1"""
    rng = np.random.default_rng(100 + seed)
    n = 4000
    seeds = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    ports = np.where(rng.random(n) < 0.2, rng.integers(0xfffffffd, 1 << 32, n), rng.integers(0, 1 << 32, n)).astype(np.uint64)
    kind = rng.integers(0, 4, n)
    index = np.where(kind == 0, rng.integers(0, 1 << 20, n, dtype=np.uint64),
                     np.where(kind == 1, np.uint64((1 << 32) - 8) + rng.integers(0, 16, n, dtype=np.uint64), rng.integers(0, 1 << 64, n, dtype=np.uint64)))
    x = rng.uniform(-1.3, 1.3, n)
    x[::5] = rng.normal(0.0, 1e-3, x[::5].size)
    scale = np.array([ref.SCALE[f] for f in FMTS])[rng.integers(0, 4, n)]
    on_half = (rng.integers(-100, 100, n) + 0.5) / scale
    x[1::7] = on_half[1::7]
    x[2::7] = np.nextafter(on_half[2::7], np.inf)
    x[3::11] = rng.choice([0.0, 1.0, -1.0, 1.0 - 2 ** -53, -1.0 + 2 ** -53], x[3::11].size)
    lines = []
    for i in range(n):
        s, p, at = int(seeds[i]), int(ports[i]), int(index[i])
        h = int(ref.hashes(s, p, at, 1)[0])
        want = [int(ref.codes(f, x[i:i + 1], s, p, at)[0]) for f in FMTS]
        lines.append("%x %x %x %x %x %d %d %d %d" % (s, p, at, int(np.float64(x[i]).view(np.uint64)), h, *want))
    table = tmp_path / "table.txt"
    table.write_text("\n".join(lines) + "\n")
    r = subprocess.run([dither_check, str(table)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "OK %d rows" % n, r.stdout + r.stderr
