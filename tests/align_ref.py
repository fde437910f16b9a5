"""The alignment record of the render report as include/gdg.h defines it, restated in numpy float64: a direct sum per lag (np.correlate
on the central slice of the reference), the same treatment of non-finite samples, the same tie rule.  Nothing here imports the library:
the tests compare the library against this."""
import numpy as np

L = 8192                         # a block
MAX_LAG = 2048
DTYPE = np.dtype([("corr", "<f8"), ("corr0", "<f8"), ("ref_sq", "<f8"), ("sq_at_lag", "<f8"), ("lag", "<i4"), ("reserved", "<u4")])


def padded(block):
    """at most L samples -> L: a short block is zero-padded, a non-finite sample is taken as 0"""
    b = np.asarray(block, dtype=np.float64)
    assert b.ndim == 1 and b.size <= L
    out = np.zeros(L)
    out[:b.size] = np.where(np.isfinite(b), b, 0.0)
    return out


def correlation(x_block, y_block, M):
    """r[l] = sum_{n=M}^{L-M-1} x[n] y[n + l] for l = -M .. M, as an array of 2M + 1 values (index l + M)"""
    assert 1 <= M <= MAX_LAG
    x, y = padded(x_block), padded(y_block)
    return np.correlate(y, x[M:L - M], mode="valid")      # 'valid': y[k : k + L - 2M] . x[M : L - M] for k = 0 .. 2M, k = l + M


def pick(r, M):
    """the l with the greatest |r[l]|; equal magnitudes go to the smaller |l|, then to the negative one"""
    lags = np.arange(-M, M + 1)
    mag = np.abs(r)
    best = np.flatnonzero(mag == mag.max())
    return int(min(lags[best], key=lambda l: (abs(l), l)))


def record(x_block, y_block, M):
    """(the record as a dict, r, sum of y^2 over the whole block: the S of the tests' bound is sqrt(ref_sq * that))"""
    x, y = padded(x_block), padded(y_block)
    r = correlation(x, y, M)
    lag = pick(r, M)
    rec = dict(corr=float(r[lag + M]), corr0=float(r[M]), ref_sq=float(np.sum(x[M:L - M] ** 2)),
               sq_at_lag=float(np.sum(y[M + lag:L - M + lag] ** 2)), lag=lag, reserved=0)
    return rec, r, float(np.sum(y * y))


def margin(r, M):
    """how far the peak of |r| stands above the runner-up at any other lag"""
    mag = np.abs(r)
    k = int(np.argmax(mag))
    return float(mag[k] - np.max(np.delete(mag, k)))


def block_align(rows, ref, M):
    """records [n_rows][blocks] (DTYPE) of equally long rows; ref[r] = -1: zeros"""
    rows = [np.asarray(r, dtype=np.float64) for r in rows]
    blocks = -(-rows[0].size // L)
    out = np.zeros((len(rows), blocks), dtype=DTYPE)
    for p, q in enumerate(ref):
        if q < 0:
            continue
        for j in range(blocks):
            rec, _, _ = record(rows[q][j * L:(j + 1) * L], rows[p][j * L:(j + 1) * L], M)
            out[p, j] = tuple(rec[k] for k in DTYPE.names)
    return out
