"""The three stand-alone blend calls run one device body, one table and one launcher (csrc/api_io.cpp, blend.h, blend_kernels.h): a list
that lacks a part gives the same bits through every call that can take it, and those bits are the numpy restatement's
(tests/blend_filter_ref.py).  3 rows, 2 blends of 1, 5 and 6 terms -- the first term alone, one unrolled group of four, a group and a
remainder; 1, 2, 513 and 4096 + 513 samples, the last across the tile from which no sample can lie in front of the launch; every base
16-byte aligned with even strides (16-byte lanes) and every base offset by one sample (8-byte lanes); with a history and without one.
Cells outside [0, samples) of a sum's row keep their fill, rows and history are read and never written.  Lists with taps, 32 terms, a
single offset base and the refusals: tests/test_gpu_blend_filter.py; the delays' edge values: tests/test_gpu_blend_delay.py."""
import numpy as np
import pytest

import blend_filter_ref as ref
from helpers import package

pytestmark = pytest.mark.gpu

MAXD = ref.MAX_DELAY
ROWS = 3
FILL = 7.0
WEIGHTS = (0.75, -1.25, 0.5, 1e-3, -0.3, 2.0)
DELAYS = (1, 0, 4096, 255, 2, 256)                  # odd and even (the pair load and the two single ones), none, the limit, both sides of a tile


def terms(K, shift, delayed):
    return [((k + shift) % ROWS, WEIGHTS[(k + shift) % 6]) + ((DELAYS[(k + shift) % 6],) if delayed else ()) for k in range(K)]


# 2 blends a list; term counts 1, 5 and 6 each come first and second
PLAIN = [[terms(a, 0, False), terms(b, 1, False)] for a, b in ((1, 5), (5, 6), (6, 1))]
DELAYED = [[terms(a, 0, True), terms(b, 1, True)] for a, b in ((1, 5), (5, 6), (6, 1))]
SAMPLES = (1, 2, 513, MAXD + 513)


@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, 8192)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def cases():
    """rows, history and the restatement's sums per sample count, computed once"""
    out = {}
    for samples in SAMPLES:
        rng = np.random.default_rng(300 + samples)
        x, hist = rng.uniform(-1.5, 1.5, (ROWS, samples)), rng.uniform(-1.5, 1.5, (ROWS, MAXD))
        x[:, ::5] *= 1e-9
        out[samples] = dict(x=x, hist=hist, plain=[ref.blends(x, b) for b in PLAIN],
                            delayed={h: [ref.blends(x, b, hist if h else None) for b in DELAYED] for h in (False, True)})
    return out


@pytest.mark.parametrize("with_history", [False, True])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("samples", SAMPLES)
def test_every_call_that_can_take_a_list_writes_the_restatement_s_bits(ctx1, cases, samples, off, with_history):
    case = cases[samples]
    x, hist = case["x"], case["hist"]
    even = samples + (samples & 1)
    d_in, d_out, d_hist = ctx1.alloc(1, ROWS * even + 2), ctx1.alloc(1, 2 * even + 2), ctx1.alloc(1, ROWS * MAXD + 2)
    padded, hp = np.full(ROWS * even + 2, 9.0), np.full(ROWS * MAXD + 2, 5.0)
    for r in range(ROWS):
        padded[off + r * even:off + r * even + samples] = x[r]
        hp[off + r * MAXD:off + (r + 1) * MAXD] = hist[r]
    d_in.upload(padded)
    d_hist.upload(hp)
    history = (d_hist.ptr + 8 * off, MAXD) if with_history else (None, MAXD)

    def run(call, blends, *hist_args):
        """the sums of one call, [2, samples]; everything around them still holds the fill"""
        d_out.upload(np.full(d_out.cols, FILL))
        call(d_in.ptr + 8 * off, even, ROWS, samples, blends, d_out.ptr + 8 * off, even, *hist_args)
        raw = d_out.download().reshape(-1)
        inside = np.zeros(raw.size, dtype=bool)
        for b in range(2):
            inside[off + b * even:off + b * even + samples] = True
        assert np.array_equal(raw[~inside], np.full(raw.size - 2 * samples, FILL)), "cells outside [0, samples) of a sum's row were written"
        return raw[inside].reshape(2, samples)

    for i, blends in enumerate(PLAIN):
        # no delays: the plain call, the delayed call with no delay list and with zeros, the filtered call with neither and with empty taps
        zeros = [[t + (0,) for t in b] for b in blends]
        empty = [[t + (0, []) for t in b] for b in blends]
        got = [run(ctx1.blend_rows_device, blends), run(ctx1.blend_rows_delayed_device, blends, *history), run(ctx1.blend_rows_delayed_device, zeros, *history),
               run(ctx1.blend_rows_filtered_device, blends, *history), run(ctx1.blend_rows_filtered_device, empty, *history)]
        for j, g in enumerate(got):
            assert g.tobytes() == got[0].tobytes(), (i, j)
        for b in range(2):
            assert ref.same_bits(got[0][b], case["plain"][i][b]), (i, b)
    for i, blends in enumerate(DELAYED):
        # delays and no taps: the delayed and the filtered call
        got = [run(ctx1.blend_rows_delayed_device, blends, *history), run(ctx1.blend_rows_filtered_device, blends, *history),
               run(ctx1.blend_rows_filtered_device, [[t + ([],) for t in b] for b in blends], *history)]
        for j, g in enumerate(got):
            assert g.tobytes() == got[0].tobytes(), (i, j)
        for b in range(2):
            assert ref.same_bits(got[0][b], case["delayed"][with_history][i][b]), (i, b)
    assert np.array_equal(d_in.download().reshape(-1), padded) and np.array_equal(d_hist.download().reshape(-1), hp)      # read, never written
    d_in.free()
    d_out.free()
    d_hist.free()
