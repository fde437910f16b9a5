"""The numpy restatement of the output trim include/gdg.h states (gdg_batch_set_trim): y = x * g in float64 -- one rounded product, numpy
never fuses -- and then the encoder's restatement applied to y: the plain encoder (clamp, scale, truncate toward zero; restated here) or the
dithered one (tests/dither_ref.py).  And the planner, gdg_trim_from_true_peak.  Nothing here calls the code under test."""
import numpy as np

import dither_ref

FORMATS = ["lpcm8", "lpcm16", "lpcm24", "lpcm32", "ieee32", "ieee64"]
WIDTH = dict(dither_ref.WIDTH, ieee32=4, ieee64=8)
SCALE = dither_ref.SCALE                       # the plain encoder's constants: 127, 32767.5, 8388607.5, 2147483647.5


def plain_codes(fmt, y):
    """the signed codes (int64) the plain LPCM encoder gives a row: trunc(S * clamp1(y)), clamped to the format's range"""
    y = np.clip(np.asarray(y, dtype=np.float64), -1.0, 1.0)
    q = np.trunc(SCALE[fmt] * y)
    lo, hi = dither_ref.RANGE[fmt]
    return np.clip(q, lo, hi).astype(np.int64)


def plain_encode(fmt, y):
    """the file's bytes (uint8 array) of a row through the plain encoder, all six formats"""
    y = np.asarray(y, dtype=np.float64)
    if fmt == "ieee64":
        return np.ascontiguousarray(y.astype("<f8")).view(np.uint8).reshape(-1)
    if fmt == "ieee32":
        return np.ascontiguousarray(np.clip(y, -1.0, 1.0).astype("<f4")).view(np.uint8).reshape(-1)
    q = plain_codes(fmt, y)
    if fmt == "lpcm8":
        return np.clip(q + 128, 0, 255).astype(np.uint8)
    return np.ascontiguousarray((q & 0xffffffff).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :WIDTH[fmt]]).reshape(-1)


def trimmed(x, g):
    """y = fl(x * g)"""
    return np.asarray(x, dtype=np.float64) * np.float64(g)


def encode(fmt, x, g, dither=None, port=0, first=0):
    """the bytes of a row of a port with gain g; dither: None (the plain encoder) or the seed (LPCM formats only: IEEE is never dithered)"""
    y = trimmed(x, g)
    if dither is None or fmt not in dither_ref.SCALE:
        return plain_encode(fmt, y)
    return dither_ref.encode(fmt, y, dither, port, first)


def plan(true_peak, target, max_gain):
    """true_peak: [ports, blocks] float64 -> the gains: 1.0 for a silent port, else min(target / max, max_gain)"""
    tp = np.asarray(true_peak, dtype=np.float64).reshape(len(true_peak), -1)
    out = np.ones(tp.shape[0])
    for p in range(tp.shape[0]):
        m = tp[p].max() if tp.shape[1] else 0.0
        if m != 0.0:
            out[p] = min(np.float64(target) / m, np.float64(max_gain))
    return out
