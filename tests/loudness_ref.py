"""The loudness records (include/gdg.h, LOUDNESS) restated in plain Python and numpy, for the tests: the K-weighting's coefficients, the
recurrence run sequentially in float64 and once more in np.longdouble, the hop sums, and the two planners.  Nothing here knows the library."""
import math

import numpy as np

SHELF = (1681.974450955533, 0.7071752369554196, 3.999843853973347, 0.4996667741545416)
HIGH_PASS = (38.13547087602444, 0.5003270373238773)
STATE_DOUBLES = 7
TILE = 8192
# ITU-R BS.1770-4, tables 1 and 2: the two stages at 48 kHz as the standard prints them
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)


def coefficients(rate):
    """shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2"""
    f0, q, g, e = SHELF
    k = math.tan(math.pi * f0 / rate)
    vh = 10.0 ** (g / 20.0)
    vb = vh ** e
    a0 = 1.0 + k / q + k * k
    out = [(vh + vb * k / q + k * k) / a0, 2.0 * (k * k - vh) / a0, (vh - vb * k / q + k * k) / a0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]
    f0, q = HIGH_PASS
    k = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + k / q + k * k
    return out + [1.0, -2.0, 1.0, 2.0 * (k * k - 1.0) / a0, (1.0 - k / q + k * k) / a0]


def high_pass_delta(rate):
    """alpha = 1 + a1 + a2 and beta = 2 + a1 of the high-pass, made without the subtraction"""
    f0, q = HIGH_PASS
    k = math.tan(math.pi * f0 / rate)
    a0 = 1.0 + k / q + k * k
    return 4.0 * k * k / a0, (2.0 * k / q + 4.0 * k * k) / a0


def hops(rate, first, count):
    h = rate // 10
    return (first + count) // h - first // h


def finite(x):
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isfinite(x), x, 0.0)


def k_weight(x, rate):
    """the recurrence of include/gdg.h, sample by sample in float64 (Python floats are IEEE doubles, every operation rounded on its own)"""
    b0, b1, b2, a1, a2 = coefficients(rate)[:5]
    alpha, beta = high_pass_delta(rate)
    s0 = s1 = q0 = q1 = 0.0
    y = [0.0] * len(x)
    for n, v in enumerate(finite(x).tolist()):
        y1 = b0 * v + s0
        s0 = (b1 * v - a1 * y1) + s1
        s1 = b2 * v - a2 * y1
        out = y1 + q0
        q0 = q0 + (q1 - beta * out)
        q1 = q1 - alpha * out
        y[n] = out
    return np.array(y, dtype=np.float64)


def k_weight_rows_longdouble(rows, rate):
    """the same recurrence with the float64 coefficients and every operation in np.longdouble, all rows at once; the outputs rounded to float64"""
    x = finite(rows).astype(np.longdouble)
    ld = np.longdouble
    b0, b1, b2, a1, a2 = [ld(c) for c in coefficients(rate)[:5]]
    alpha, beta = [ld(c) for c in high_pass_delta(rate)]
    n_rows, n = x.shape
    s0, s1, q0, q1 = (np.zeros(n_rows, dtype=ld) for _ in range(4))
    y = np.zeros((n_rows, n), dtype=ld)
    for i in range(n):
        v = x[:, i]
        y1 = b0 * v + s0
        s0 = (b1 * v - a1 * y1) + s1
        s1 = b2 * v - a2 * y1
        out = y1 + q0
        q0 = q0 + (q1 - beta * out)
        q1 = q1 - alpha * out
        y[:, i] = out
    return y.astype(np.float64)


def hop_sums(y, rate, exact=False):
    """the whole hops of a K-weighted row: squares in float64; summed in np.longdouble (exact) or sequentially in float64"""
    h = rate // 10
    n = len(y) // h
    sq = (np.asarray(y, dtype=np.float64) ** 2)[:n * h].reshape(n, h)
    if exact:
        return sq.astype(np.longdouble).sum(axis=1)
    return np.array([_seq_sum(r) for r in sq.tolist()], dtype=np.float64)


def _seq_sum(values):
    acc = 0.0
    for v in values:
        acc += v
    return acc


def lufs(power):
    return -0.691 + 10.0 * math.log10(power) if power > 0.0 else -math.inf


def from_hops(records, rate, ports, weights=None):
    """(integrated, momentary_max, short_term_max) of the programme made of `ports` of records [ports][hops] with their channel weights"""
    rec = np.asarray(records, dtype=np.float64)
    h = rate // 10
    w = [1.0] * len(ports) if weights is None else list(weights)
    z = np.zeros(rec.shape[1])
    for p, g in zip(ports, w):
        z = z + g * rec[p] / h
    blocks = np.array([(z[j] + z[j + 1] + z[j + 2] + z[j + 3]) / 4.0 for j in range(max(0, len(z) - 3))])
    momentary = lufs(blocks.max()) if len(blocks) else -math.inf
    short = [z[j:j + 30].sum() / 30.0 for j in range(max(0, len(z) - 29))]
    short_term = lufs(max(short)) if short else -math.inf
    above = blocks[blocks > 10.0 ** ((-70.0 + 0.691) / 10.0)] if len(blocks) else blocks
    if len(above) == 0:
        return -math.inf, momentary, short_term
    rel = above.mean() * 10.0 ** (-10.0 / 10.0)
    kept = above[above > rel]
    return (lufs(kept.mean()) if len(kept) else -math.inf), momentary, short_term


def trim_from_loudness(records, rate, target_lufs, ceiling_dbtp=0.0, true_peak=None):
    """(gain, capped) per port: toward the target, capped where the port's largest true peak times the gain would pass the ceiling"""
    rec = np.asarray(records, dtype=np.float64)
    gain, capped = np.ones(rec.shape[0]), np.zeros(rec.shape[0], dtype=bool)
    for p in range(rec.shape[0]):
        level = from_hops(rec, rate, [p])[0]
        if math.isfinite(level):
            gain[p] = 10.0 ** ((target_lufs - level) / 20.0)
        if true_peak is not None:
            m = float(np.max(true_peak[p])) if np.size(true_peak[p]) else 0.0
            if m > 0.0 and 10.0 ** (ceiling_dbtp / 20.0) / m < gain[p]:
                gain[p], capped[p] = 10.0 ** (ceiling_dbtp / 20.0) / m, True
    return gain, capped
