"""The delivery (include/gdg.h, DELIVERY) without a GPU: the numpy restatement (tests/deliver_ref.py) against its known answers and against
the reference's semantics -- oracle.OversamplerDecimator(R).decimate fed in 8192-sample blocks, at the project's parity bar of 1e-9 RMS --;
the byte counts of a delivered step as a program of its own (tests/native/deliver_bytes_check.cpp), once more under the address and
undefined-behaviour sanitizers; and the compiler's resource summary of the kernels.

Where the reference defines the comparison at factor 2.  oversampling.Decimate runs its anti-aliasing filter through filter.Process, and
filter.Process clips every sample it EMITS to [-1, 1] (filter/filter.go:473-503; oracle/filter.c, "clip only what is emitted") -- before
Decimate multiplies by ATTENUATION_HALF_DECIBEL.  The 2x filter passes 80 % of the band, so full-scale uniform noise leaves it above 1.0 at
some samples (10 to 16 per 4096 delivered samples with seed 1); there the reference gives exactly +-A and the direct sum gives A f with
|f| > 1, up to 0.21 apart.  The 4x filter passes 40 % of the band and the same noise never reaches 1.0.  The delivery does not clip (the
encoders do), so the comparison is pinned where |f| <= 1, and the samples with |f| > 1 are held to be exactly +-A: that is the cause, not
a tolerance."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import deliver_ref as ref

ROOT = entry.ROOT
CSRC = os.path.join(entry.PKG_DIR, "csrc")
BLOCK = 8192
PARITY_RMS = 1e-9                                                           # the project's parity bar


@pytest.fixture(scope="module")
def oracle():
    o = entry.load_oracle()
    o.build()
    return o


def test_the_restated_taps_are_the_reference_tables(oracle):
    for factor in (2, 4):
        h = ref.taps(factor)
        assert h.size == ref.TAPS[factor] and np.array_equal(h, h[::-1])
        assert np.array_equal(h, oracle.aa_taps(factor))
        assert ref.LATENCY[factor] == (h.size - 1) // 2 and int(np.argmax(h)) == ref.LATENCY[factor]
    assert ref.HISTORY == ref.TAPS[4] - 1


@pytest.mark.parametrize("factor", [2, 4])
def test_known_answers(factor):
    h = ref.taps(factor)
    n = factor * 100
    for at in (0, 1):
        x = np.zeros(n)
        x[at] = 1.0
        y = ref.deliver(x, factor)
        assert y.size == n // factor
        for i in range(y.size):
            k = factor * i - at
            assert y[i] == (ref.A * h[k] if 0 <= k < h.size else 0.0), (factor, at, i)
    y = ref.deliver(np.zeros(n), factor)
    assert not y.any() and not np.signbit(y).any()                          # silence: exactly +0.0
    x = np.random.default_rng(5).uniform(-1, 1, 2 * n)                       # continued through the history: the same bits
    hist = ref.next_history(x[:n])
    assert np.array_equal(np.concatenate([ref.deliver(x[:n], factor), ref.deliver(x[n:], factor, hist)]), ref.deliver(x, factor))
    short = ref.next_history(x[:10], hist)                                   # fewer than 154: the old ones move up
    assert np.array_equal(short[0, :-10], hist[0, 10:]) and np.array_equal(short[0, -10:], x[:10])


@pytest.mark.parametrize("factor", [2, 4])
def test_impulses_against_the_reference(oracle, factor):
    """the test of record for the taps and the phase: impulses at sample 0 and at sample 1"""
    for at in (0, 1):
        x = np.zeros(BLOCK)
        x[at] = 1.0
        got = oracle.OversamplerDecimator(factor).decimate(x)
        want = ref.deliver(x, factor)
        worst = float(np.abs(got - want).max())
        print("factor %d, impulse at %d: max |oracle - restatement| = %.3e" % (factor, at, worst))
        # the reference convolves through 256- and 512-point transforms: log2(512) = 9 stages there and back, each within an ulp of values
        # below 0.43 (the largest tap): 2 * 9 * 2^-53 * 0.43 < 1e-15.  A tap off by one place would show at 1e-6 or more.
        assert worst <= 1e-15, (factor, at, worst)


@pytest.mark.parametrize("factor", [2, 4])
def test_noise_against_the_reference_where_it_defines_it(oracle, factor):
    x = np.random.default_rng(1).uniform(-1.0, 1.0, 4 * BLOCK)
    dec = oracle.OversamplerDecimator(factor)
    got = np.concatenate([dec.decimate(x[b * BLOCK:(b + 1) * BLOCK]) for b in range(4)])
    want = ref.deliver(x, factor)
    f = want / ref.A
    clipped = np.abs(f) > 1.0 + 1e-12                                        # the filter's output leaves [-1, 1]: the reference emits +-1
    inside = np.abs(f) < 1.0 - 1e-12
    assert np.count_nonzero(clipped) + np.count_nonzero(inside) == f.size    # no sample of this input sits on the edge
    rms = float(np.sqrt(np.mean((got[inside] - want[inside]) ** 2)))
    print("factor %d: RMS %.3e (max %.3e) over %d samples inside, %d clipped by the reference's filter" % (
        factor, rms, np.abs(got[inside] - want[inside]).max(), np.count_nonzero(inside), np.count_nonzero(clipped)))
    assert rms <= PARITY_RMS
    assert np.array_equal(got[clipped], ref.A * np.sign(f[clipped]))        # ... and there exactly +-A: the clip is the whole difference
    if factor == 4:
        assert not clipped.any()                                            # the whole comparison: every sample of factor 4
    else:
        assert clipped.any() and float(np.abs(got - want).max()) > 0.1       # the issue's isolated samples, up to 0.2 apart


def test_the_byte_counts_as_a_stand_alone_program(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "deliver_bytes_check.cpp")
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("deliver_bytes_check_" + name))
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, src, "-o", exe], check=True, timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.match(r"OK delivered step bytes; (\d+) step cases\n", r.stdout)
        assert m and int(m.group(1)) == 120, r.stdout + r.stderr


def design_table():
    """the resources table of DESIGN.md 4.12i: {kernel: (VGPRs, scratch, LDS bytes)}"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    part = text[text.index("### 4.12i"):]
    rows = re.findall(r"^\| `(deliver\w+(?:<[^>]*>)?)` \| (\d+) \| (\d+) \| ([\d ]+) \|", part, re.M)
    return {name: (int(v), int(s), int(lds.replace(" ", ""))) for name, v, s, lds in rows}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_kernels_use_no_scratch_and_the_lds_of_the_table(tmp_path):
    """deliver_rows_kernel<R> (both load paths) and deliver_history_save_kernel from the compiler's resource summary of io.hip: no scratch; LDS
    of R * 256 + T - 1 doubles rounded up to whole phases, the figures DESIGN.md 4.12i states; VGPRs that leave eight waves per SIMD."""
    out = str(tmp_path / "io.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "io.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"\.amdhsa_kernel (_Z\w*deliver\w+)\n.*?^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    rows = {n: f for n, f in found.items() if "deliver_rows_kernel" in n}
    assert len(rows) == 4 and len(found) == 5, sorted(found)
    table = design_table()
    for name, (vgprs, scratch, lds) in found.items():
        assert scratch == 0 and vgprs <= 64, (name, vgprs, scratch)
        if "deliver_rows_kernel" in name:
            R = 2 if "ILi2E" in name else 4
            assert lds == 8 * R * -(-(R * 256 + ref.TAPS[R] - 1) // R), (name, lds)
            assert table["deliver_rows_kernel<%d>" % R] == (vgprs, 0, lds), (name, table)
        else:
            assert lds == 0 and table["deliver_history_save_kernel"] == (vgprs, 0, 0), (name, table)
    # every product and add on its own: no fused multiply-add in the kernels' text
    for m in re.finditer(r"^(_Z\w*deliver_rows_kernel\w+):.*?\.amdhsa_kernel", text, re.S | re.M):
        assert "v_fma_f64" not in m.group(0), m.group(1)
