"""The three paths of the batch block loop that tests/test_gpu_records_one_chain.py (5 blocks in windows of 4, 6 encoded rows) never reaches, in
the smallest job that reaches all of them: the helper thread that gathers a step's inputs (a window of 4 blocks or more and more than 3 steps),
the opening quarter and half windows (a window of 8 or more and a job of three windows or more), and the download in four pieces (a step of
4 blocks or more and 8 encoded rows or more).  4 channels at 48 kHz, 29 blocks less a ragged tail in windows of 8 -- steps of 2, 4, 8, 8, 4, 2
and 1 blocks -- with one blend that reaches back (8 encoded rows), delivered at a half of the rate and 147/160 of that, TPDF dither, a trim,
all nine record kinds on, one input at another rate (the resampler's carry crosses steps) and one channel that reads another's source (the
fan-out descriptors).  The job run in one call and streamed in slices of 13 and 16 blocks (steps of 2, 4, 4, 2, 1 | 1, 8, 4, 2, 1) writes the
same files and keeps the same records, byte for byte."""
import numpy as np
import pytest

from helpers import package, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
RATE, OTHER_RATE, NCH, BLOCKS, WINDOW = 48000, 44100, 4, 29, 8
SLICES = (13, 16)
SAMPLES = (BLOCKS - 1) * BLOCK + 1000
NO = NCH + 3
NR = NO + 1
DELIVERY = (2, 147, 160)
BLENDS = [[(0, 0.6, 37), (1, -0.4)]]                                            # port NO; its first term reads 37 samples back
SOURCES = [0, 1, 2, 0]                                                          # channel 3 reads channel 0's input
TRIM = ([0.5, -0.75, 1.25, 0.9], 0.8, 0.7, 1.1)
DITHER_SEED = 20240607
# kind -> (what switches it on, its getter, the axis of its records that counts blocks)
KINDS = {
    "stats": (lambda ctx: ctx.batch_report_enable(True), "batch_report", 1),
    "spectrum": (lambda ctx: ctx.batch_spectrum_enable([100.0, 1000.0, 5000.0, 20000.0]), "batch_spectrum", 1),
    "align": (lambda ctx: ctx.batch_align_enable([-1, 0, -1, -1, -1, -1, -1, 0], 64), "batch_align", 1),
    "true_peak": (lambda ctx: ctx.batch_true_peak_enable(True), "batch_true_peak", 1),
    "fit": (lambda ctx: ctx.batch_fit_enable([(NO, [0, 1])]), "batch_fit", 1),
    "gram": (lambda ctx: ctx.batch_gram_enable([0, NCH, NO]), "batch_gram", 0),
    "tapfit": (lambda ctx: ctx.batch_tapfit_enable([(0, [1], 4)]), "batch_tapfit", 0),
    "transfer": (lambda ctx: ctx.batch_transfer_enable([(0, 1)], 32), "batch_transfer", 0),
    "delivered": (lambda ctx: ctx.batch_delivered_enable(True), "batch_delivered", 1),
}


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


def inputs():
    """channel 1 at another rate, a little shorter than the job; channel 3 has no entry of its own"""
    out = []
    for c in range(NCH):
        rate = OTHER_RATE if c == 1 else RATE
        out.append((lpcm16_file(0.5 * synth_signal(c, SAMPLES * rate // RATE, rate)), "lpcm16", rate))
    out[3] = None
    return out


def configured(pkg):
    ctx = pkg.Context(NCH, BLOCK)
    for c in range(NCH):
        if c % 2 == 0:
            ctx.append_unit(c, "overdrive", params=[0, 20, 100, 0, 1, 2])
        else:
            ctx.append_unit(c, "tone_stack")
    ctx.spatializer_set_sample_rate(RATE)
    for c in range(NCH):
        ctx.spatializer_set_position(c, -40.0 + 25.0 * c, 1.0 + 0.5 * c, 0.8)
    ctx.set_window(WINDOW)
    ctx.batch_set_sources(SOURCES)
    ctx.batch_set_blends(BLENDS)
    ctx.batch_set_delivery_ratio(*DELIVERY)
    ctx.batch_set_dither(1, DITHER_SEED, 0)
    ctx.batch_set_trim(*TRIM)
    for enable, _getter, _axis in KINDS.values():
        enable(ctx)
    return ctx


def records(ctx):
    return {kind: getattr(ctx, getter)().copy() for kind, (_enable, getter, _axis) in KINDS.items()}


def test_one_call_and_slices_of_13_and_16_blocks_write_the_same_files_and_records():
    pkg = package()
    ins = inputs()
    ctx = configured(pkg)
    whole = [o.tobytes() for o in ctx.batch_run(ins, RATE, "lpcm24")]
    whole_rec = records(ctx)
    ctx.close()

    ctx = configured(pkg)
    left = list(SLICES)
    pieces, slice_rec = [], []
    for outs in ctx.batch_stream(ins, RATE, "lpcm24", lambda _left: left.pop(0)):
        pieces.append([o.tobytes() for o in outs])
        slice_rec.append(records(ctx))
    ctx.close()

    assert len(whole) == NR and len(pieces) == len(SLICES) and all(len(p) == NR for p in pieces)
    assert len({len(f) for f in whole}) == 1 and len(whole[0]) > 0
    for r in range(NR):
        assert whole[r].strip(b"\0"), "output %d is all zeros" % r
        assert b"".join(p[r] for p in pieces) == whole[r], "output %d: the slices against the one call" % r
    for kind, (_enable, _getter, axis) in KINDS.items():
        a = whole_rec[kind]
        b = np.concatenate([s[kind] for s in slice_rec], axis=axis)
        assert a.shape[axis] == BLOCKS and [s[kind].shape[axis] for s in slice_rec] == list(SLICES), kind
        assert a.tobytes().strip(b"\0"), "%s: the records are all zeros" % kind
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), "%s: the slices' records against the one call's" % kind
