"""The true-peak record of the render report as include/gdg.h defines it, restated in numpy float64.  Nothing here imports the library: the
tap table is an argument (formula_taps() builds one from the definition; the tests hand over the library's own to compare bits).  A point
is acc = acc + x[n + j] * h[j] over j in ascending order from 0.0, vectorised over n: numpy does not fuse separate operations."""
import numpy as np

L = 8192                         # a block
OS = 4                           # the oversampling factor
H = 12                           # the half-width: 24 taps per phase
DTYPE = np.dtype([("true_peak", "<f8"), ("position", "<u4"), ("overs", "<u4")])


def formula_taps():
    """h[p - 1][j + H - 1] for p = 1, 2, 3 and j = -H + 1 .. H"""
    out = np.zeros((OS - 1, 2 * H))
    for p in range(1, OS):
        t = p / OS - np.arange(-H + 1, H + 1, dtype=np.float64)
        g = np.sin(np.pi * t) / (np.pi * t) * (0.5 + 0.5 * np.cos(np.pi * t / H))
        s = 0.0
        for v in g:                                      # the normalising sum in ascending j
            s = s + v
        out[p - 1] = g / s
    return out


def points(block, taps):
    """the cleaned samples x[l] and the interpolated values v[3][count] for n = H - 1 .. l - H - 1 (count = 0 when l < 24)"""
    x = np.asarray(block, dtype=np.float64)
    assert x.ndim == 1 and x.size <= L
    x = np.where(np.isfinite(x), x, 0.0)
    count = max(0, x.size - 2 * H + 1)
    v = np.zeros((OS - 1, count))
    for p in range(OS - 1):
        acc = np.zeros(count)
        for k in range(2 * H):                           # k = j + H - 1: sample n + j = (n - H + 1) + k, n - H + 1 = 0 .. count - 1
            acc = acc + x[k:k + count] * taps[p][k]
        v[p] = acc
    return x, v


def magnitudes(block, taps):
    """|value| at every position 4 n + p of the block, -1 where no point is evaluated"""
    x, v = points(block, taps)
    mag = np.full(4 * max(x.size, 1), -1.0)
    mag[0:4 * x.size:4] = np.abs(x)
    for p in range(OS - 1):
        n = np.arange(v.shape[1]) + H - 1
        mag[4 * n + p + 1] = np.abs(v[p])
    return mag, v


def record(block, taps):
    """(true_peak, position, overs) of one block of at most L samples"""
    mag, v = magnitudes(block, taps)
    peak = float(mag.max()) if mag.size else 0.0
    if not peak > 0.0:
        return 0.0, 0, int(np.count_nonzero(np.abs(v) > 1.0))
    return peak, int(np.flatnonzero(mag == peak)[0]), int(np.count_nonzero(np.abs(v) > 1.0))


def runner_up(block, taps):
    """the largest magnitude at any position other than the record's, relative to the maximum (1.0: a tie)"""
    mag, _ = magnitudes(block, taps)
    k = int(np.argmax(mag))
    rest = np.delete(mag, k)
    return float(rest.max() / mag[k]) if mag[k] > 0.0 and rest.size else 0.0


def block_true_peak(rows, taps):
    """records [n_rows][blocks] (DTYPE) of equally long rows"""
    rows = [np.asarray(r, dtype=np.float64) for r in rows]
    blocks = -(-rows[0].size // L)
    out = np.zeros((len(rows), blocks), dtype=DTYPE)
    for r, row in enumerate(rows):
        for b in range(blocks):
            out[r, b] = record(row[b * L:(b + 1) * L], taps)
    return out
