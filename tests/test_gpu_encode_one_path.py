"""The plain, the dithered and the trimmed encoder kernels are started by three launchers, one per form, that pick the kernel from a
gdg_encode_mode (csrc/io.hip, the encode launchers): the seams of that fold, byte for byte.  The stand-alone device form in every valid (format, mode) -- six plain,
four dithered, six trimmed, four trimmed and dithered -- at 1, 3, 4, 5, 7 and 8 samples (the tail alone, exactly one group of four, a group
and a tail) with aligned buffers, the samples offset by 8 bytes (everything through the tail kernel) and the bytes offset by 1, against the
numpy restatements (tests/trim_ref.py, tests/dither_ref.py); the host form against the device form; the master finish of two shards and aux
on one group of four samples, its sums kept and not kept; and the rows form in the smallest batch job, with a blend port whose launch has
gains of its own.  The finish and the rows are held against the stand-alone call on the float64 values they encode.  Gain 1.0 goes down the
delegation trim -> dither -> plain, so one call reaches all four modes.  Whole files, windows, slices, shards, refusals:
tests/test_gpu_io.py, test_gpu_dither.py, test_gpu_trim.py."""
import numpy as np
import pytest

import dither_ref
import trim_ref as ref
from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
SEED, PORT, FIRST = 0x7219a5c3e1d0f864, 7, 2 ** 40 + 1
GAIN = -1.7
# +-1, past full scale, -0.0, 0.1 and 1/3 (their products with -1.7 round), small values the dither decides
X = np.array([1.0, -1.0, 1.3, -0.0, 0.1, -1.2, 1.0 / 3.0, 1e-5])
# (format, mode, gain): plain, dithered, trimmed, trimmed and dithered -- an IEEE format is never dithered
COMBOS = ([(f, 0, 1.0) for f in ref.FORMATS] + [(f, 1, 1.0) for f in dither_ref.SCALE] +
          [(f, 0, GAIN) for f in ref.FORMATS] + [(f, 1, GAIN) for f in dither_ref.SCALE])
MODES = [(0, False), (1, False), (0, True), (1, True)]                      # (dither mode, trimmed)
assert len(COMBOS) == 20 and X.size == 8


def want_bytes(fmt, x, gain, mode, port=PORT, first=FIRST):
    return ref.encode(fmt, x, gain, SEED if mode else None, port, first)


@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


def device_form(ctx, d_in, d_out, fmt, n, gain, mode, in_off=0, out_off=0):
    """x[:n] at d_in + in_off -> the n * width bytes at d_out + out_off, and that nothing else of d_out was written"""
    lib, w = package().lib(), ref.WIDTH[fmt]
    d_in.upload(np.concatenate([[9.0] * (in_off // 8), X[:n], [9.0] * (d_in.cols - n - in_off // 8)]))
    d_out.upload(np.zeros(d_out.cols))
    ctx.wave_encode_trim_device(fmt, d_in.ptr + in_off, n, d_out.ptr + out_off, gain, mode, SEED, PORT, FIRST)
    raw = np.zeros(d_out.cols * 8, dtype=np.uint8)
    ctx._check(lib.gdg_copy_to_host(ctx._h, raw.ctypes.data, d_out.ptr, raw.size))
    assert not raw[:out_off].any() and not raw[out_off + n * w:].any(), "bytes outside the output were written"
    return raw[out_off:out_off + n * w]


@pytest.mark.parametrize("in_off,out_off", [(0, 0), (8, 0), (0, 1)])
def test_the_device_form_writes_the_restatement_s_bytes(ctx1, in_off, out_off):
    d_in, d_out = ctx1.alloc(1, X.size + 2), ctx1.alloc(1, X.size + 2)
    for fmt, mode, gain in COMBOS:
        for n in (1, 3, 4, 5, 7, 8):
            got = device_form(ctx1, d_in, d_out, fmt, n, gain, mode, in_off, out_off)
            assert np.array_equal(got, want_bytes(fmt, X[:n], gain, mode)), (fmt, mode, gain, n, in_off, out_off)
    d_in.free()
    d_out.free()


def test_the_host_form_is_the_device_form(ctx1):
    d_in, d_out = ctx1.alloc(1, X.size + 2), ctx1.alloc(1, X.size + 2)
    for fmt, mode, gain in COMBOS:
        dev = device_form(ctx1, d_in, d_out, fmt, 7, gain, mode).copy()
        assert np.array_equal(ctx1.wave_encode_trim(fmt, X[:7], gain, mode, SEED, PORT, FIRST), dev), (fmt, mode, gain)
    d_in.free()
    d_out.free()


@pytest.mark.parametrize("keep_sums", [False, True])
def test_the_master_finish_encodes_its_sums_as_the_stand_alone_call_does(ctx1, keep_sums):
    """two shards and aux, one group of four samples; the sums in the kernel's order, (p_0 + p_1) + aux, which numpy's adds restate"""
    rng = np.random.default_rng(71)
    lefts, rights, aux = [rng.uniform(-0.6, 0.6, 4) for _ in range(2)], [rng.uniform(-0.6, 0.6, 4) for _ in range(2)], rng.uniform(-0.3, 0.3, 4)
    lefts[0][0], rights[1][3] = 0.1, 1.0 / 3.0
    sums = [(lefts[0] + lefts[1]) + aux, (rights[0] + rights[1]) + aux]
    gains, ports = (GAIN, 0.5), (dither_ref.PORT_LEFT, dither_ref.PORT_RIGHT)
    ctx = package().Context(1, BLOCK)
    ctx.batch_report_enable(keep_sums)
    for mode, trimmed in MODES:
        ctx.batch_set_dither(mode, SEED, 0)
        ctx.batch_set_trim([1.0], *((gains + (1.0,)) if trimmed else (1.0, 1.0, 1.0)))
        for fmt in (dither_ref.SCALE if mode else ref.FORMATS):
            got = ctx.batch_finish_master(fmt, lefts, rights, aux=aux)
            for side in range(2):
                want = ctx1.wave_encode_trim(fmt, sums[side], gains[side] if trimmed else 1.0, mode, SEED, ports[side], 0)
                assert np.array_equal(got[side], want), (fmt, mode, trimmed, side)
                assert np.array_equal(want, ref.encode(fmt, sums[side], gains[side] if trimmed else 1.0, SEED if mode else None, ports[side], 0))
            if keep_sums:                                                   # the records read the sums the kernel kept: untrimmed
                report = ctx.batch_report()
                assert report.shape == (2, 1)
                for side in range(2):
                    assert report["peak"][side, 0] == np.abs(sums[side]).max() and report["peak_index"][side, 0] == np.abs(sums[side]).argmax(), (fmt, mode, trimmed, side)
                    # every sample of the kept row: four samples are two pairs on two lanes, summed pair by pair and then lane 0 + lane 1
                    q = sums[side] * sums[side]
                    assert report["sum_sq"][side, 0] == (q[0] + q[1]) + (q[2] + q[3]), (fmt, mode, trimmed, side)
    ctx.close()


def test_the_rows_form_encodes_its_rows_as_the_stand_alone_call_does(ctx1):
    """one channel, one block, a blend port: chain, master left and right, metronome in one launch, the blend in a second with its own gain"""
    pkg = package()
    x = 0.1 * synth_signal(0, BLOCK, 48000)
    inputs = [(np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8), "lpcm16", 48000)]
    gains = [GAIN, 0.5, -1.0, 3.0, 1.7]                                      # chain 0, master left, right, metronome, the blend
    ports = [0, dither_ref.PORT_LEFT, dither_ref.PORT_RIGHT, dither_ref.PORT_METRONOME, 4]

    def run(fmt, mode, trimmed):
        ctx = pkg.Context(1, BLOCK)
        ctx.append_unit(0, "power_amp", fir=synth_ir(300, seed=80))
        ctx.spatializer_set_sample_rate(48000)
        ctx.spatializer_set_position(0, -20.0, 1.5, 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
        ctx.metronome_configure(4, 150, 48000)
        ctx.batch_set_blends([[(0, 0.75)]], gain=[gains[4]] if trimmed else None)
        ctx.batch_set_dither(mode, SEED, 0)
        if trimmed:
            ctx.batch_set_trim(gains[:1], *gains[1:4])
        outs = ctx.batch_run(inputs, 48000, fmt, metronome_to_master=True)
        ctx.close()
        return outs

    rows = [o.view(np.float64) for o in run("ieee64", 0, False)]
    assert len(rows) == 5 and all(r.size == BLOCK and r.any() for r in rows)
    for mode, trimmed in MODES:
        outs = run("lpcm24", mode, trimmed)
        for r in range(5):
            want = ctx1.wave_encode_trim("lpcm24", rows[r], gains[r] if trimmed else 1.0, mode, SEED, ports[r], 0)
            assert np.array_equal(outs[r], want), (mode, trimmed, r, np.count_nonzero(outs[r] != want))
