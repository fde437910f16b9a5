"""The numpy restatement of the filtered blend outputs include/gdg.h states (FILTERS: gdg_batch_set_blends_filtered,
gdg_blend_rows_filtered): a term is (channel, weight[, delay[, taps]]); without taps x_k[i] = x[c_k][i - d_k], with taps f = h[0] * x[c_k][i
- d_k], then f = f + (h[t] * x[c_k][i - d_k - t]) in ascending t; s = w_0 * x_0, then s = s + (w_k * x_k) in term order -- numpy rounds every
float64 product and every add on its own and never fuses or reorders them.  The samples in front of sample 0 come from the row's history or
are +0.0.  And the restatements of the two host planners: the windowed-sinc taps of a fractional delay and the fraction from fit records.
Nothing here calls the code under test."""
import numpy as np

import blend_delay_ref as delay_ref

MAX_DELAY = delay_ref.MAX_DELAY
MAX_TAPS = 64
same_bits = delay_ref.same_bits


def reach(term):
    """how far back a term reads: d + max(T, 1) - 1"""
    d = term[2] if len(term) > 2 else 0
    T = len(term[3]) if len(term) > 3 and term[3] is not None else 0
    return d + max(T, 1) - 1


def filtered_row(row, d, taps, history=None):
    """x_k of one term: the row read d samples back, through its taps where it has some"""
    row = np.asarray(row, dtype=np.float64)
    h = np.zeros(0) if taps is None else np.asarray(taps, dtype=np.float64).reshape(-1)
    if h.size == 0:
        return delay_ref.delayed_row(row, d, history)
    assert h.size <= MAX_TAPS and d + h.size - 1 <= MAX_DELAY
    with np.errstate(all="ignore"):
        f = h[0] * delay_ref.delayed_row(row, d, history)
        for t in range(1, h.size):
            f = f + h[t] * delay_ref.delayed_row(row, d + t, history)
    return f


def blend(rows, terms, history=None):
    """rows: [n_rows, samples] float64; terms: [(channel, weight[, delay[, taps]]), ..]; history: None or [n_rows, MAX_DELAY]"""
    rows = np.asarray(rows, dtype=np.float64)
    x = lambda t: filtered_row(rows[t[0]], t[2] if len(t) > 2 else 0, t[3] if len(t) > 3 else None, None if history is None else history[t[0]])
    with np.errstate(all="ignore"):
        s = np.float64(terms[0][1]) * x(terms[0])
        for t in terms[1:]:
            s = s + np.float64(t[1]) * x(t)
    return s


def blends(rows, lists, history=None):
    """[blends, samples]: one row per list of terms"""
    return np.stack([blend(rows, t, history) for t in lists])


def fraction_taps(T, f):
    """T taps (even) that delay by T/2 - 1 + f samples: sinc(u) (0.5 + 0.5 cos(2 pi u / T)), u = t - (T/2 - 1) - f, over their sum"""
    assert T % 2 == 0 and 2 <= T <= MAX_TAPS and 0.0 <= f < 1.0
    if f == 0.0:
        h = np.zeros(T)
        h[T // 2 - 1] = 1.0
        return h
    u = np.arange(T, dtype=np.float64) - (T // 2 - 1) - f
    h = np.sin(np.pi * u) / (np.pi * u) * (0.5 + 0.5 * np.cos(2.0 * np.pi * u / T))
    total = 0.0
    for v in h:
        total += float(v)
    return h / total


def fraction_step(records, steps):
    """the winner of one fit's records (a structured array with tt, tx, xx, terms over the blocks): k - (steps - 1) of the candidate with the
    largest tx[k] / sqrt(xx[k][k]) among those with xx[k][k] > 0, the earlier on a tie; 0 where tt <= 0 or none is admissible"""
    K = 2 * steps - 1
    tt, tx, xx = 0.0, [0.0] * K, [0.0] * K
    for r in records:
        assert int(r["terms"]) == K
        tt += float(r["tt"])
        for k in range(K):
            tx[k] += float(r["tx"][k])
            xx[k] += float(r["xx"][k * (k + 1) // 2 + k])
    if not tt > 0.0:
        return 0
    best, score = -1, 0.0
    for k in range(K):
        if not xx[k] > 0.0:
            continue
        v = tx[k] / np.sqrt(xx[k])
        if best < 0 or v > score:
            best, score = k, v
    return 0 if best < 0 else best - (steps - 1)
