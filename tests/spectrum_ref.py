"""The band spectrum of the render report as include/gdg.h defines it, restated in numpy float64 (numpy.fft.rfft plus the k_lo rule).
Nothing here imports the library: the tests compare the library against this."""
import numpy as np

L = 8192                         # a block = the transform
BINS = L // 2 + 1                # k = 0 .. L/2


def window():
    """w[n] = 0.5 - 0.5 cos(2 pi n / L): the periodic Hann window"""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / L)


def k_lo(edges_hz, sample_rate):
    """clamp((long long)ceil(edge * 8192.0 / R), 0, 4097), in float64 as written"""
    e = np.asarray(edges_hz, dtype=np.float64)
    with np.errstate(over="ignore"):
        k = np.ceil(e * 8192.0 / np.float64(sample_rate))
    return np.clip(k, 0.0, float(BINS)).astype(np.int64)


def bin_powers(block):
    """P[k], k = 0 .. L/2, of one block (at most L samples: a short one is zero-padded; a non-finite sample is taken as 0)"""
    b = np.asarray(block, dtype=np.float64)
    assert b.ndim == 1 and b.size <= L
    x = np.zeros(L)
    x[:b.size] = np.where(np.isfinite(b), b, 0.0)
    X = np.fft.rfft(window() * x)
    c = np.full(BINS, 2.0)
    c[0] = c[L // 2] = 1.0
    return c * (X.real * X.real + X.imag * X.imag) / (float(L) * float(L) * 3.0 / 8.0)


def bands_of(powers, edges_hz, sample_rate):
    """band b = the sum of P[k] over k_lo[b] <= k < k_lo[b + 1]; a band without a bin is exactly 0.0"""
    lo = k_lo(edges_hz, sample_rate)
    return np.array([powers[lo[i]:lo[i + 1]].sum() if lo[i + 1] > lo[i] else 0.0 for i in range(lo.size - 1)])


def block_spectrum(row, sample_rate, edges_hz):
    """(bands [blocks][n_bands], totals [blocks]) of one row; totals = the sum over ALL bins of each block (the T of the tests' bound)"""
    row = np.asarray(row, dtype=np.float64)
    blocks = -(-row.size // L)
    out = np.zeros((blocks, len(edges_hz) - 1))
    tot = np.zeros(blocks)
    for j in range(blocks):
        p = bin_powers(row[j * L:(j + 1) * L])
        out[j] = bands_of(p, edges_hz, sample_rate)
        tot[j] = p.sum()
    return out, tot
