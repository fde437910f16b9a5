"""The records of the delivered rows (include/gdg.h, DELIVERED RECORDS) restated in numpy, operation by operation: the pair-walk order of the
sum of squares (thread t of 256 takes the pairs t, t + 256, ..; the wave tree + 32 .. + 1; the four wave sums in wave order) and the 24-tap
sums one product and one add at a time, from 0.0 in ascending tap order.  numpy's elementwise multiply and add round each operation on its
own, so every figure here has the bits the definition asks for."""
import numpy as np

DTYPE = np.dtype([("true_peak", "<f8"), ("peak", "<f8"), ("sum_sq", "<f8"), ("position", "<i4"), ("peak_index", "<u4"), ("overs", "<u4"), ("clipped", "<u4")])
H = 12
TAPS = 24
HISTORY = 23
THREADS = 256


def finite(x):
    """a non-finite sample is taken as 0"""
    x = np.array(x, dtype=np.float64)
    x[~np.isfinite(x)] = 0.0
    return x


def sum_sq(x):
    """sum of x[i]^2 in block_stats_kernel's order at L = len(x)"""
    L = x.size
    rounds = -(-L // (2 * THREADS))
    sq = np.zeros(rounds * 2 * THREADS)
    sq[:L] = x * x
    sq = sq.reshape(rounds, THREADS, 2)
    acc = np.zeros(THREADS)
    for r in range(rounds):                     # a padded slot adds +0.0, which changes no bit of a sum that is never -0.0
        acc = acc + sq[r, :, 0]
        acc = acc + sq[r, :, 1]
    waves = acc.reshape(4, 64)
    o = 32
    while o:
        waves = waves[:, :o] + waves[:, o:2 * o]
        o //= 2
    w = waves[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def points(lead, x, taps):
    """v[p][c] for the intervals that end with the block's samples c = 0 .. L - 1: interval n = c - 12 reads lead ++ x at c .. c + 23"""
    ext = np.concatenate([lead, x])
    L = x.size
    v = np.zeros((3, L))
    for p in range(3):
        acc = np.zeros(L)
        for k in range(TAPS):
            acc = acc + ext[k:k + L] * taps[p, k]
        v[p] = acc
    return v


def record(lead, x, taps):
    """one block: x its samples, lead the 23 in front of them (both already finite)"""
    rec = np.zeros((), dtype=DTYPE)
    L = x.size
    mag = np.abs(x)
    i = int(np.argmax(mag))                       # the first largest
    rec["peak"], rec["peak_index"] = mag[i], i
    rec["sum_sq"] = sum_sq(x)
    rec["clipped"] = int(np.count_nonzero(mag > 1.0))
    v = np.abs(points(lead, x, taps))
    rec["overs"] = int(np.count_nonzero(v > 1.0))
    best, pos = mag[i], 4 * i
    m = v.max()
    if m >= best:
        p, c = np.nonzero(v == m)
        q = int((4 * (c - H) + p + 1).min())
        if m > best or q < pos:
            best, pos = m, q
    rec["true_peak"] = best
    rec["position"] = pos if best > 0.0 else 0
    return rec


def block_delivered(rows, span, taps, history=None):
    """rows [n_rows][samples] cut by span[0 .. n_blocks] -> [n_rows][n_blocks] records; history: None (zeros in front) or [n_rows][23], which is
    UPDATED IN PLACE to the last 23 samples of (history ++ rows), as the library's call does"""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    span = [int(s) for s in span]
    taps = np.asarray(taps, dtype=np.float64).reshape(3, TAPS)
    out = np.zeros((rows.shape[0], len(span) - 1), dtype=DTYPE)
    for r in range(rows.shape[0]):
        front = np.zeros(HISTORY) if history is None else history[r]
        ext = finite(np.concatenate([front, rows[r]]))
        for k in range(len(span) - 1):
            o, e = span[k], span[k + 1]
            out[r, k] = record(ext[o:o + HISTORY], ext[HISTORY + o:HISTORY + e], taps)
        if history is not None:
            history[r] = np.concatenate([front, rows[r]])[-HISTORY:]
    return out


def spans(factor, up, down, first_block, blocks, out_samples):
    """the delivered blocks of the session blocks [first_block, first_block + blocks), relative to the first: span[j] = N(8192 (first_block + j)) -
    N(8192 first_block), N(s) = out_samples(factor, up, down, 0, s)"""
    base = out_samples(factor, up, down, 0, 8192 * first_block)
    return [out_samples(factor, up, down, 0, 8192 * (first_block + j)) - base for j in range(blocks + 1)]
