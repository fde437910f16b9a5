"""The numpy restatement of the delayed blend outputs include/gdg.h states (gdg_batch_set_blends_delayed, gdg_blend_rows_delayed):
x_k[i] = x[c_k][i - d_k], the samples in front of sample 0 taken from the row's history or +0.0; s = w_0 * x_0, then s = s + (w_k * x_k) in
term order -- numpy rounds every float64 product and every add on its own and never fuses or reorders them.  Nothing here calls the code
under test."""
import numpy as np

MAX_DELAY = 4096


def delayed_row(row, d, history=None):
    """the row read d samples back: its first d samples are the last d of `history` ([MAX_DELAY], the last entry is sample -1), or +0.0"""
    row = np.asarray(row, dtype=np.float64)
    assert 0 <= d <= MAX_DELAY
    if d == 0:
        return row
    front = np.zeros(d) if history is None else np.asarray(history, dtype=np.float64)[MAX_DELAY - d:]
    return np.concatenate([front, row])[:row.size]


def blend(rows, terms, history=None):
    """rows: [n_rows, samples] float64; terms: [(channel, weight) or (channel, weight, delay), ..]; history: None or [n_rows, MAX_DELAY]"""
    rows = np.asarray(rows, dtype=np.float64)
    x = lambda t: delayed_row(rows[t[0]], t[2] if len(t) > 2 else 0, None if history is None else history[t[0]])
    with np.errstate(all="ignore"):
        s = np.float64(terms[0][1]) * x(terms[0])
        for t in terms[1:]:
            s = s + np.float64(t[1]) * x(t)
    return s


def blends(rows, lists, history=None):
    """[blends, samples]: one row per list of terms"""
    return np.stack([blend(rows, t, history) for t in lists])


def same_bits(got, want):
    """== on the bits of every sample that is a number; a NaN answers a NaN (include/gdg.h leaves its sign and payload open)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)))


def port_lag(records, min_coeff):
    """lag and sign of one port from its alignment records (a structured array with corr, ref_sq, sq_at_lag, lag), as the header states"""
    lags, total = [], 0.0
    for r in records:
        if not (r["ref_sq"] > 0 and r["sq_at_lag"] > 0):
            continue
        if not abs(r["corr"]) / np.sqrt(r["ref_sq"] * r["sq_at_lag"]) >= min_coeff:
            continue
        lags.append(int(r["lag"]))
        total += float(r["corr"])
    if not lags:
        return 0, 1
    return sorted(lags)[(len(lags) - 1) // 2], (-1 if total < 0 else 1)
