"""The numpy restatement of the blend outputs include/gdg.h states (gdg_batch_set_blends, gdg_blend_rows): s = w_0 * x[c_0], then
s = s + (w_k * x[c_k]) in term order -- numpy rounds every float64 product and every add on its own and never fuses or reorders them.
Nothing here calls the code under test."""
import numpy as np


def blend(rows, terms):
    """rows: [n_rows, samples] float64; terms: [(channel, weight), ..] -> the blend's float64 row"""
    rows = np.asarray(rows, dtype=np.float64)
    with np.errstate(all="ignore"):
        c, w = terms[0]
        s = np.float64(w) * rows[c]
        for c, w in terms[1:]:
            s = s + np.float64(w) * rows[c]
    return s


def blends(rows, lists):
    """[blends, samples]: one row per list of terms"""
    return np.stack([blend(rows, t) for t in lists])


def same_bits(got, want):
    """== on the bits of every sample that is a number; a NaN answers a NaN -- its sign and payload are nothing IEEE 754 defines (0 * inf is
    the negative quiet NaN on x86 and the positive one on gfx950)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)))
