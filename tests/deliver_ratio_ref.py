"""The ratio stage of the delivery (include/gdg.h, DELIVERY, "a rational ratio behind the factor") restated in numpy, from the header's text
alone: the prototype from its formula, the outputs, the counts and the history by plain loops in float64.

    T = 2 * ceil(32 * max(1, M / L));  g[m] = L * 2 fc * sinc(2 fc u) * I0(beta * sqrt(1 - (u / c)^2)) / I0(beta),  u = m - c, c = L T / 2,
    fc = 0.5 / max(L, M), beta = 10;  tap[p][t] = g[p + t L]
    output n: b = floor(n M / L), p = (n M) mod L;  f = tap[p][0] x[b];  f = f + tap[p][t] x[b - t], t = 1 .. T - 1 ascending

numpy multiplies and adds float64 arrays element by element with one rounding each (no fused multiply-add), so running the t loop over whole
arrays performs, for every n, exactly the stated sequence.  Indices are Python integers: no floating point and no overflow."""
from math import gcd

import numpy as np

HISTORY = 127
BETA = 10.0


def admissible(up, down):
    return 1 <= up <= 160 and 1 <= down <= 320 and down <= 2 * up and up <= 2 * down and gcd(up, down) == 1


def tap_count(up, down):
    """T = 2 * ceil(32 * max(1, M / L)) in integers"""
    return 64 if down <= up else 2 * -(-32 * down // up)


def latency(factor, up, down):
    """session samples a delivered port lags the render by: the factor's (T - 1) / 2 and R * T / 2 of the ratio stage"""
    return {1: 0, 2: 38, 4: 77}[factor] + (factor * tap_count(up, down) // 2 if (up, down) != (1, 1) else 0)


def prototype(up, down):
    """g[m], m = 0 .. L T - 1, from the formula (np.i0 is a Chebyshev fit: another route to I0 than the library's power series)"""
    L, T = up, tap_count(up, down)
    fc = 0.5 / max(up, down)
    c = L * T / 2.0
    u = np.arange(L * T, dtype=np.float64) - c
    return L * 2.0 * fc * np.sinc(2.0 * fc * u) * np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (u / c) ** 2))) / np.i0(BETA)


def table(up, down):
    """tap[p][t] = g[p + t L], as [L][T]"""
    return np.ascontiguousarray(prototype(up, down).reshape(tap_count(up, down), up).T)


def first_out(s, up, down):
    """ceil(s L / M): the first output that does not lie in front of intermediate sample s"""
    return -(-s * up // down)


def count(first, samples, up, down):
    return first_out(first + samples, up, down) - first_out(first, up, down)


def delivered_samples(factor, up, down, first, n):
    """gdg_batch_out_samples by exact integer arithmetic: session samples [first, first + n), both multiples of factor"""
    return count(first // factor, n // factor, up, down)


def deliver(x, up, down, first=0, history=None, taps=None):
    """One row (1-D) or rows (2-D) of intermediate samples, the job's [first, first + samples) -> their outputs.  history: None or [..., 127],
    the samples in front of x (the newest last).  taps: the [L][T] table to use (the library's own, for the bit-for-bit comparisons)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        return deliver(x[None, :], up, down, first, None if history is None else np.asarray(history).reshape(1, HISTORY), taps)[0]
    if (up, down) == (1, 1):
        return x.copy()
    tap = table(up, down) if taps is None else np.asarray(taps, dtype=np.float64).reshape(up, -1)
    T = tap.shape[1]
    assert T == tap_count(up, down)
    rows, samples = x.shape
    front = np.zeros((rows, HISTORY)) if history is None else np.asarray(history, dtype=np.float64).reshape(rows, HISTORY)
    ext = np.concatenate([front, x], axis=1)                    # ext[:, HISTORY + s] = x[:, s]; T - 1 <= 127
    n0, n1 = first_out(first, up, down), first_out(first + samples, up, down)
    n = [n0 + j for j in range(n1 - n0)]
    at = np.array([HISTORY + (k * down // up - first) for k in n], dtype=np.int64)
    p = np.array([(k * down) % up for k in n], dtype=np.int64)
    if not n:
        return np.zeros((rows, 0))
    assert at.min() >= HISTORY and at.max() < HISTORY + samples
    f = tap[p, 0] * ext[:, at]
    for t in range(1, T):
        f = f + (tap[p, t] * ext[:, at - t])
    return f


def next_history(x, history=None):
    """What the history holds after a call on x: the last 127 samples of [history | x]."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x[None, :]
    front = np.zeros((x.shape[0], HISTORY)) if history is None else np.asarray(history, dtype=np.float64).reshape(x.shape[0], HISTORY)
    return np.concatenate([front, x], axis=1)[:, -HISTORY:]


def rate_triple(session, delivered):
    """(factor, up, down) for a (session rate, delivered rate) pair: of the admissible ones the ratio closest to 1; None where there is none"""
    found = []
    for factor in (1, 2, 4):
        if session % factor:
            continue
        g = gcd(delivered, session // factor)
        up, down = delivered // g, session // factor // g
        if admissible(up, down):
            found.append((max(up, down) / min(up, down), (factor, up, down)))
    return min(found)[1] if found else None


def gain_db(g, up, f_over_nyquist, lower):
    """|G(f)| / L in dB of the prototype g (which runs at L times the intermediate rate) at f = f_over_nyquist times the Nyquist frequency of the
    lower rate: that frequency is 0.5 / max(L, M) cycles per prototype sample."""
    w = 2.0 * np.pi * np.asarray(f_over_nyquist, dtype=np.float64) * 0.5 / lower
    m = np.arange(g.size, dtype=np.float64)
    h = np.array([abs(np.sum(g * np.exp(-1j * wk * m))) for wk in np.atleast_1d(w)]) / up
    return 20.0 * np.log10(np.maximum(h, 1e-300))
