"""A numpy float64 restatement of the transfer record (include/gdg.h, TRANSFER) and of its planner: np.fft.fft on the windowed blocks, the
group sums in the normative order (ascending k, plain adds from +0.0), np.fft.irfft for the planner.  Shared by the host and the GPU tests."""
import numpy as np

L = 8192
H = L // 2
SCALE = float(L) * float(L) * 3.0 / 8.0
GROUPS = (1, 2, 4, 8, 16, 32, 64)


def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / L)


def groups(D):
    return H // D + 1


def doubles(n_pairs, D):
    return n_pairs * groups(D) * 4


def group_bins(g, D):
    """the bins of group g, clipped to 0 .. 4096 (both ends included)"""
    return max(g * D - (D - 1) // 2, 0), min(g * D + D // 2, H)


def finite(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isfinite(x), x, 0.0)


def block_of(row, b):
    out = np.zeros(L)
    part = finite(row[b * L:(b + 1) * L])
    out[:part.size] = part
    return out


def bins(x, y):
    """the per-bin values of one block pair: Pxx, Pyy, Re Pxy, Im Pxy for k = 0 .. 4096"""
    w = window()
    X, Y = np.fft.fft(w * x)[:H + 1], np.fft.fft(w * y)[:H + 1]
    P = np.conj(X) * Y / SCALE
    im = P.imag.copy()
    im[0] = im[H] = 0.0
    return np.stack([np.abs(X) ** 2 / SCALE, np.abs(Y) ** 2 / SCALE, P.real, im], axis=1)


def grouped(per_bin, D):
    """[4097, 4] -> [G, 4]: ascending k, one add at a time from +0.0"""
    G = groups(D)
    out = np.zeros((G, 4))
    for g in range(G):
        lo, hi = group_bins(g, D)
        acc = np.zeros(4)
        for k in range(lo, hi + 1):
            acc = acc + per_bin[k]
        out[g] = acc
    return out


def record(rows, pairs, D):
    """rows [n_rows, samples] -> [blocks, n_pairs, G, 4]"""
    rows = np.asarray(rows, dtype=np.float64)
    blocks = -(-rows.shape[1] // L)
    out = np.zeros((blocks, len(pairs), groups(D), 4))
    cache = {}
    for b in range(blocks):
        for i, (p, t) in enumerate(pairs):
            if (b, p, t) not in cache:
                cache[(b, p, t)] = bins(block_of(rows[p], b), block_of(rows[t], b))
            out[b, i] = grouped(cache[(b, p, t)], D)
    return out


def totals(rows, pairs):
    """per block and pair the tolerance scales: sum Pxx, sum Pyy, sqrt of their product (twice: both parts of Sxy) -> [blocks, n_pairs, 1, 4]"""
    rows = np.asarray(rows, dtype=np.float64)
    blocks = -(-rows.shape[1] // L)
    out = np.zeros((blocks, len(pairs), 1, 4))
    for b in range(blocks):
        for i, (p, t) in enumerate(pairs):
            v = bins(block_of(rows[p], b), block_of(rows[t], b))
            sx, sy = v[:, 0].sum(), v[:, 1].sum()
            out[b, i, 0] = [sx, sy, np.sqrt(sx * sy), np.sqrt(sx * sy)]
    return out


def taper(n_taps, center):
    m = np.arange(n_taps) - center
    E = np.where(m < 0, center + 1.0, float(n_taps - center))
    return 0.5 + 0.5 * np.cos(np.pi * m / E)


def plan(records, n_pairs, D, n_taps, center=0, ridge=0.0):
    """records [blocks, n_pairs x G x 4] (any shape of that size per block) -> (taps [n_pairs, n_taps], coherence [n_pairs])"""
    G = groups(D)
    Gm = G - 1
    M = 2 * Gm
    rec = np.asarray(records, dtype=np.float64).reshape(-1, n_pairs, G, 4)
    taps, coh = np.zeros((n_pairs, n_taps)), np.zeros(n_pairs)
    for p in range(n_pairs):
        s = np.zeros((G, 4))
        for q in range(rec.shape[0]):
            s = s + rec[q, p]
        sxx, syy, sxy = s[:, 0], s[:, 1], s[:, 2] + 1j * s[:, 3]
        den = sxx + ridge * (sxx.sum() / G)
        Hg = np.where(den != 0.0, sxy / np.where(den != 0.0, den, 1.0), 0.0)
        Hg[0], Hg[Gm] = Hg[0].real, Hg[Gm].real
        h = np.fft.irfft(Hg, M)
        idx = (np.arange(n_taps) - center) % M
        taps[p] = taper(n_taps, center) * h[idx]
        on = sxx > 0.0
        coh[p] = (np.abs(sxy[on]) ** 2 / sxx[on]).sum() / syy.sum() if syy.sum() > 0.0 else 0.0
    return taps, coh


def synth_records(h, D, blocks=1):
    """records of one pair whose port is white (Sxx = 1) and whose target is the port through the filter h: Syy = |H|^2, Sxy = H at g / N'"""
    G = groups(D)
    M = 2 * (G - 1)
    Hg = np.array([np.sum(np.asarray(h, dtype=np.float64) * np.exp(-2j * np.pi * g * np.arange(len(h)) / M)) for g in range(G)])
    rec = np.zeros((blocks, 1, G, 4))
    rec[..., 0] = 1.0 / blocks
    rec[..., 1] = np.abs(Hg) ** 2 / blocks
    rec[..., 2] = Hg.real / blocks
    rec[..., 3] = Hg.imag / blocks
    rec[:, 0, 0, 3] = rec[:, 0, G - 1, 3] = 0.0
    return rec
