"""The CPU side of the band spectrum (include/gdg.h, gdg_block_spectrum_rows): the four entry points in every layer, the definition's
known answers in its numpy restatement (tests/spectrum_ref.py), the k_lo rule -- in numpy and, through a stand-alone program under
AddressSanitizer and UBSan, in the host code the library uses (csrc/spectrum_bands.h) --, the wrapper's refusals, and the kernel's
registers, scratch and LDS from the compiler's own summary.  What the kernel computes is tests/test_gpu_block_spectrum.py's business."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import spectrum_ref as ref

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
NAMES = ("gdg_block_spectrum_rows", "gdg_block_spectrum_rows_device", "gdg_batch_spectrum_enable", "gdg_batch_spectrum")
RATES = (44100, 48000, 192000)


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_header_carries_the_prototypes_and_the_library_exports_them(pkg):
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = " ".join(f.read().split())
    for proto in ("int gdg_block_spectrum_rows(gdg_ctx *ctx, const double *const *rows, int n_rows, size_t samples, uint32_t sample_rate, "
                  "const double *edges_hz, int n_edges, double *bands);",
                  "int gdg_block_spectrum_rows_device(gdg_ctx *ctx, const double *d_rows, size_t row_stride, int n_rows, size_t samples, "
                  "uint32_t sample_rate, const double *edges_hz, int n_edges, double *d_bands);",
                  "int gdg_batch_spectrum_enable(gdg_ctx *ctx, const double *edges_hz, int n_edges);",
                  "int gdg_batch_spectrum(gdg_ctx *ctx, double *bands, size_t capacity, int *ports, size_t *blocks, int *n_bands);"):
        assert proto in header, proto
    for phrase in ("0.5 - 0.5 cos(2 pi n / L)", "c_k |X[k]|^2 / (L^2 * 3/8)", "clamp((long long)ceil(edges[b] * 8192.0 / R), 0, 4097)",
                   "A^2/3 into its own bin and A^2/12 into each neighbour", "is exactly 0.0"):
        assert phrase in header.replace(" * ", " ").replace("edges[b] 8192.0", "edges[b] * 8192.0").replace("(L^2 3/8)", "(L^2 * 3/8)"), phrase
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for n in NAMES:
        assert n in exported and n in pkg.ABI_SYMBOLS and getattr(pkg.lib(), n).argtypes is not None, n
    for m in ("block_spectrum", "block_spectrum_device", "batch_spectrum_enable", "batch_spectrum"):
        assert callable(getattr(pkg.Context, m)), m
    base = os.path.dirname(os.path.dirname(pkg.LIB_PATH))
    with open(os.path.join(base, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    for fn, sym in zip(("BlockSpectrumRows", "BlockSpectrumRowsDevice", "BatchSpectrumEnable", "BatchSpectrum"), NAMES):
        assert re.search(r"^func \(this \*Context\) %s\(" % fn, go, re.M) and "C.%s(" % sym in go, fn


def test_known_answers_hold_in_the_restatement():
    """a sine of amplitude 0.5 at bin 100, the bins 99, 100 and 101 in three bands of their own: 0.25/12, 0.25/3, 0.25/12; the total A^2/2;
    Parseval: the sum over all bins is the windowed block's mean square over 3/8"""
    rate = 48000
    # the phase is reduced in integers: every sample is the sine of an angle below 2 pi, rounded once (angles up to 200 pi carry their own
    # rounding into the samples, which alone moves the neighbours' power by 1.7e-15 relative)
    x = 0.5 * np.sin(2.0 * np.pi * ((100 * np.arange(ref.L)) % ref.L) / ref.L)
    hz = lambda k: k * rate / 8192.0
    edges = [hz(98.5), hz(99.5), hz(100.5), hz(101.5)]
    assert list(ref.k_lo(edges, rate)) == [99, 100, 101, 102]
    bands, tot = ref.block_spectrum(x, rate, edges)
    for got, want in zip(bands[0], (0.25 / 12.0, 0.25 / 3.0, 0.25 / 12.0)):
        assert abs(got - want) <= 1e-15 * want, (got, want)
    assert abs(tot[0] - 0.125) <= 1e-14 * 0.125
    noise = np.random.default_rng(3).standard_normal(ref.L)
    p = ref.bin_powers(noise)
    want = float(np.sum((ref.window() * noise) ** 2)) / (ref.L * 3.0 / 8.0)
    assert abs(p.sum() - want) <= 1e-13 * want
    assert np.all(ref.bin_powers(np.zeros(100)) == 0.0)
    both = ref.bin_powers(np.array([0.25, np.nan, -0.5, np.inf, -np.inf]))
    assert np.array_equal(both, ref.bin_powers(np.array([0.25, 0.0, -0.5, 0.0, 0.0])))


@pytest.mark.parametrize("rate", RATES)
def test_k_lo_rule(rate):
    """an edge exactly on a bin, one ulp below a bin, above Nyquist, and 0"""
    for k in (1, 100, 1365, 4095, 4096):
        on = k * rate / 8192.0                                       # exact: a product by rate over a power of two
        assert on * 8192.0 / rate == k
        assert ref.k_lo([on], rate)[0] == k, "an edge exactly on bin %d belongs to that bin" % k
        below = np.nextafter(on, 0.0)
        assert ref.k_lo([below], rate)[0] == k                       # one ulp below still rounds up to k: ceil of anything in (k - 1, k]
        above = np.nextafter(on, np.inf)
        assert ref.k_lo([above], rate)[0] == (k + 1 if above * 8192.0 / rate > k else k)
    assert ref.k_lo([0.0], rate)[0] == 0
    assert list(ref.k_lo([rate / 2.0, np.nextafter(rate / 2.0, np.inf), rate * 0.75, 1e300, 1.7e308], rate)) == [4096, 4097, 4097, 4097, 4097]
    p = np.arange(ref.BINS, dtype=np.float64)
    got = ref.bands_of(p, [0.0, rate / 8192.0 * 0.25, rate / 8192.0 * 0.75, rate / 8192.0, rate / 2.0, rate, 2.0 * rate], rate)
    # bins [0, 1), [1, 1) -- two edges inside one bin --, [1, 1), [1, 4096), [4096, 4097), nothing above Nyquist
    assert list(got) == [0.0, 0.0, 0.0, float(np.arange(1, 4096).sum()), 4096.0, 0.0]


@pytest.fixture(scope="module")
def spectrum_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spectrum") / "spectrum_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "spectrum_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


def test_host_code_agrees_with_the_restatement_under_sanitizers(spectrum_check):
    """csrc/spectrum_bands.h: the refusals by hand in the program; here its k_lo for a list of edges and rates against numpy's, and its
    window table against numpy's to 1 ulp of 1 (two libms)"""
    edges = [0.0, 5e-324, 22.1, 100 * 48000 / 8192.0, float(np.nextafter(100 * 48000 / 8192.0, 0.0)), 1000.0, 11025.0, 22050.0, 24000.0,
             float(np.nextafter(24000.0, np.inf)), 96000.0, 1e12, 1e300, 1.7e308]
    for rate in RATES + (1, 4294967295):
        r = subprocess.run([spectrum_check, str(rate)] + [float(e).hex() for e in edges], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
        got = [int(v) for v in r.stdout.split()[1:1 + len(edges)]]
        assert got == list(ref.k_lo(edges, rate)), rate
    w = np.array([float.fromhex(v) for v in r.stdout.split()[1 + len(edges):]])
    assert w.size == ref.L and np.max(np.abs(w - ref.window())) <= 2.0 ** -52 and w[0] == 0.0 and w[ref.L // 2] == 1.0


@pytest.mark.parametrize("bad", [[100.0, 50.0], [10.0, 10.0], [10.0, float("nan")], [10.0, float("inf")], [-1.0, 5.0], [100.0], [],
                                 [float(i) for i in range(34)]])
def test_the_wrapper_refuses_bad_edge_lists_before_any_call(pkg, bad):
    """descending, equal, NaN, infinite, negative, one edge, none, 34 edges: refused in Python -- no context, hence no call, is involved"""
    with pytest.raises(ValueError):
        pkg.spectrum_edges(bad)
    ghost = object.__new__(pkg.Context)                              # a context that was never created: any call through it would fail otherwise
    with pytest.raises(ValueError):
        pkg.Context.block_spectrum(ghost, np.zeros(16), 48000, bad)
    if bad:
        with pytest.raises(ValueError):
            pkg.Context.batch_spectrum_enable(ghost, bad)
    assert pkg.spectrum_edges([float(i) for i in range(33)]).size == 33 and pkg.spectrum_edges([0.0, 1.0]).size == 2


def test_the_c_calls_refuse_no_context(pkg):
    e = np.array([10.0, 20.0])
    assert pkg.lib().gdg_batch_spectrum_enable(None, e.ctypes.data, 2) == pkg.GDG_ERR_INVALID
    assert pkg.lib().gdg_batch_spectrum(None, None, 0, None, None, None) == pkg.GDG_ERR_INVALID
    assert pkg.lib().gdg_block_spectrum_rows(None, None, 0, 0, 48000, e.ctypes.data, 2, None) == pkg.GDG_ERR_INVALID
    assert pkg.lib().gdg_block_spectrum_rows_device(None, None, 0, 0, 0, 48000, e.ctypes.data, 2, None) == pkg.GDG_ERR_INVALID


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_kernel_fits_two_workgroups_per_cu_without_scratch(tmp_path):
    """256 threads and two workgroups per CU: 2 waves per SIMD, so at most 256 vector registers, accumulation registers included; LDS at
    most 80 KiB; no scratch"""
    out = str(tmp_path / "fir.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "fir.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @.*?^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        if "block_spectrum_kernel" in m.group(1):
            found[m.group(1)] = tuple(int(m.group(i)) for i in (2, 3, 4))
    assert len(found) == 2, sorted(found)                            # pair loads and single loads
    for name, (vgprs, scratch, lds) in found.items():
        assert vgprs <= 256 and scratch == 0 and lds <= 80 * 1024, (name, vgprs, scratch, lds)
