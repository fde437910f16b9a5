"""The blend outputs (gdg_batch_set_blends, gdg_blend_rows) on the device, bit for bit against the numpy restatement of the arithmetic
include/gdg.h states (tests/blend_ref.py).  The stand-alone form over random rows with infinities and NaNs planted: every sample count at
which a lane's path changes, even and odd strides, 1 to 32 terms.  The batch form: three blend ports behind the metronome's in all six
formats, plain, dithered and with output gains, against the existing restatements of the encoders applied to the blends of the call's own
IEEE64 chain files; windows, slices, a source map, a resumed checkpoint; all four record kinds against the stand-alone record calls; and that
ports 0 .. N + 2, and a context with the blends taken back, are those of a context that never heard of the call."""
import numpy as np
import pytest

import blend_ref as ref
import dither_ref
import trim_ref
from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
RATE, NCH, SEED = 48000, 3, 0x5b1e2d903c47a6f8
SAMPLES, BLOCKS = 2 * BLOCK + 100, 3
NO = NCH + 3
BLENDS = [[(0, 1.0)], [(0, 0.6), (1, 0.4)], [(2, -1.0), (0, 0.1), (1, 0.2), (2, 0.3)]]
NB = len(BLENDS)
GAIN = [0.5, -1.7, 1.0]
EDGES = [100.0, 400.0, 1600.0, 6400.0]
LEVEL = 0.1


# ---- the stand-alone form ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


def random_rows(n_rows, samples, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, (n_rows, samples))
    x[:, ::7] *= 1e-9
    for v in (np.inf, -np.inf, np.nan):
        x[rng.integers(n_rows), rng.integers(samples)] = v
    return x


def term_lists(n_rows, seed):
    """1, 2, 5 and 32 terms; a channel named twice; and a zero weight (on row 0, where the caller plants an infinity)"""
    rng = np.random.default_rng(seed)
    lists = [[(int(rng.integers(n_rows)), float(rng.uniform(-2, 2))) for _ in range(k)] for k in (1, 2, 5, 32)]
    lists.append([(1, 0.6), (2, 0.25), (1, -0.4)])
    lists.append([(0, 0.0), (1, 1.0)])
    return lists


@pytest.mark.parametrize("samples", [1, 3, 4, 5, 8191, 8193])
def test_standalone_sums_are_the_restatement(ctx1, samples):
    x = random_rows(6, samples, 100 + samples)
    x[0, samples // 2] = np.inf                                             # under the zero weight of the last list: 0 * inf is NaN
    lists = term_lists(6, 7)
    want = ref.blends(x, lists)
    assert np.isnan(want[-1][samples // 2]) and np.isfinite(want[-1]).sum() >= samples - 4
    got = ctx1.blend_rows(x, lists)
    for b in range(len(lists)):
        assert ref.same_bits(got[b], want[b]), (samples, b)
    # the device form: even and odd strides on either side, the rows 16-byte aligned and 8 bytes off
    for stride, out_stride, off in ((samples + (samples & 1), samples + (samples & 1), 0), (samples | 1, samples + (samples & 1), 0),
                                    (samples + (samples & 1), samples | 1, 0), (samples + (samples & 1) + 2, samples + (samples & 1), 1)):
        d_in, d_out = ctx1.alloc(1, 6 * stride + 2), ctx1.alloc(1, len(lists) * out_stride + 2)
        padded = np.full(6 * stride + 2, 9.0)
        for r in range(6):
            padded[off + r * stride:off + r * stride + samples] = x[r]
        d_in.upload(padded)
        d_out.upload(np.full(d_out.cols, 7.0))
        ctx1.blend_rows_device(d_in.ptr + 8 * off, stride, 6, samples, lists, d_out.ptr, out_stride)
        raw = d_out.download().reshape(-1)
        for b in range(len(lists)):
            assert ref.same_bits(raw[b * out_stride:b * out_stride + samples], want[b]), (samples, stride, out_stride, off, b)
            tail = raw[b * out_stride + samples:(b + 1) * out_stride]
            assert np.array_equal(tail, np.full(tail.size, 7.0)), "samples outside a blend's row were written"
        assert np.array_equal(raw[len(lists) * out_stride:], [7.0, 7.0])
        d_in.free()
        d_out.free()


def test_known_answer_and_term_order(ctx1):
    ones = np.ones((3, 5))
    got = ctx1.blend_rows(ones, [[(0, 0.1), (1, 0.2), (2, 0.3)], [(2, 0.3), (1, 0.2), (0, 0.1)]])
    assert np.array_equal(got[0], np.full(5, 0.6000000000000001)) and np.array_equal(got[1], np.full(5, 0.6))


def test_standalone_refusals_name_blend_and_term(ctx1):
    pkg = package()
    x = np.ones((2, 4))
    for lists, what in (([[(0, 1.0)], []], "blend 1 has no term"), ([[(0, 1.0)] * 33], "33 terms"), ([[(0, 1.0), (2, 1.0)]], "blend 0, term 1"),
                        ([[(0, 1.0)], [(1, float("nan"))]], "blend 1, term 0")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx1.blend_rows(x, lists)
        assert e.value.code == pkg.GDG_ERR_INVALID


# ---- the batch form ----------------------------------------------------------------------------------------------------------------------
def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """3 channels with short chains -- a 300-tap power amp, a 64-tap one, a 128-tap one on the file of channel 0 (so the job can be described
    with a source map); 2 * 8192 + 100 samples: 3 blocks; window 2."""

    def __init__(self):
        self.pkg = package()
        files = [lpcm16_file(LEVEL * synth_signal(c, SAMPLES, RATE)) for c in range(2)]
        self.inputs = [(files[0], "lpcm16", RATE), (files[1], "lpcm16", RATE), (files[0], "lpcm16", RATE)]
        self.irs = [synth_ir(n, seed=90 + c) for c, n in enumerate((300, 64, 128))]
        self.cache = {}

    def configured(self, window=2):
        ctx = self.pkg.Context(NCH, BLOCK)
        for c in range(NCH):
            ctx.append_unit(c, "power_amp", fir=self.irs[c])
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(NCH):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * c, 1.0 + 0.5 * c, 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
        ctx.metronome_configure(4, 150, RATE)
        ctx.set_window(window)
        return ctx

    def setup(self, ctx, blends, gain, dither, records=False, align=None):
        if dither is not None:
            ctx.batch_set_dither(1, dither, 0)
        if blends is not None:
            ctx.batch_set_blends(blends, gain)
        if records:
            ctx.batch_report_enable()
            ctx.batch_spectrum_enable(EDGES)
            ctx.batch_align_enable(align if align is not None else [-1, 0, 0, -1, NCH, -1], 64)
            ctx.batch_true_peak_enable()

    def run(self, fmt, blends=BLENDS, gain=None, dither=None, records=False, align=None):
        key = (fmt, None if blends is None else len(blends), None if gain is None else tuple(gain), dither, records, None if align is None else tuple(align))
        if key not in self.cache:
            ctx = self.configured()
            self.setup(ctx, blends, gain, dither, records, align)
            outs = ctx.batch_run(self.inputs, RATE, fmt)
            res = dict(outs=outs, kib=ctx.get_option("stat_batch_device_kib"))
            if records:
                res.update(report=ctx.batch_report(), spectrum=ctx.batch_spectrum(), align=ctx.batch_align(), true_peak=ctx.batch_true_peak())
            ctx.close()
            self.cache[key] = res
        return self.cache[key]

    def rows(self):
        """the float64 chain rows and blend rows of the job: the IEEE64 files of ONE call with blends on (their bytes are the rows)"""
        outs = self.run("ieee64")["outs"]
        assert len(outs) == NO + NB
        rows = [o.view(np.float64) for o in outs]
        assert all(r.size == BLOCKS * BLOCK for r in rows) and all(np.isfinite(r).all() and r.any() for r in rows[:NCH])
        return rows


@pytest.fixture(scope="module")
def job():
    return Job()


def test_ieee64_blend_files_are_the_restatement_of_the_call_s_own_chain_files(job):
    rows = job.rows()
    want = ref.blends(np.stack(rows[:NCH]), BLENDS)
    for b in range(NB):
        assert ref.same_bits(rows[NO + b], want[b]), b
    assert not np.array_equal(rows[NO + 1], rows[0]) and not np.array_equal(rows[NO + 2], rows[NO + 1])
    assert job.run("ieee64")["kib"] > job.run("ieee64", blends=None)["kib"]      # the blend rows are counted by stat_batch_device_kib


@pytest.mark.parametrize("fmt", trim_ref.FORMATS)
def test_the_one_term_unit_blend_is_channel_0_s_file_and_the_other_ports_are_untouched(job, fmt):
    on, never = job.run(fmt), job.run(fmt, blends=None)
    assert len(on["outs"]) == NO + NB and len(never["outs"]) == NO
    assert np.array_equal(on["outs"][NO], on["outs"][0]), fmt
    for r in range(NO):
        assert np.array_equal(on["outs"][r], never["outs"][r]), (fmt, r)


@pytest.mark.parametrize("fmt", ["lpcm16", "lpcm24", "lpcm32", "ieee32"])
def test_encoded_blend_files_are_the_reference_encoders_on_the_blend_rows(job, fmt):
    rows = job.rows()
    for gain, dither in ((None, None), (None, SEED), (GAIN, None), (GAIN, SEED)):
        outs = job.run(fmt, gain=gain, dither=dither)["outs"]
        base = job.run(fmt, blends=None, dither=dither)["outs"]
        for r in range(NO):
            assert np.array_equal(outs[r], base[r]), (fmt, gain, dither, r)
        for b in range(NB):
            g = 1.0 if gain is None else gain[b]
            want = trim_ref.encode(fmt, rows[NO + b], g, dither, NO + b, 0)       # the dither's port of blend b: port_base + N + 3 + b
            assert outs[NO + b].size == want.size and np.array_equal(outs[NO + b], want), "%s, gain %s, dither %s, blend %d: %d bytes differ" % (
                fmt, g, dither is not None, b, np.count_nonzero(outs[NO + b] != want))
    if fmt in dither_ref.SCALE:
        assert not np.array_equal(job.run(fmt, gain=GAIN)["outs"][NO], job.run(fmt)["outs"][NO])


FMT = "lpcm24"


def test_windows_slices_and_a_source_map_write_the_same_bytes(job):
    want = job.run(FMT, gain=GAIN, dither=SEED)["outs"]
    for window in (1, 16):
        ctx = job.configured(window=window)
        job.setup(ctx, BLENDS, GAIN, SEED)
        got = ctx.batch_run(job.inputs, RATE, FMT)
        ctx.close()
        for r in range(NO + NB):
            assert np.array_equal(got[r], want[r]), "window %d, output %d" % (window, r)
    ctx = job.configured()
    job.setup(ctx, BLENDS, GAIN, SEED)
    parts = list(ctx.batch_stream(job.inputs, RATE, FMT, 1))
    ctx.close()
    assert len(parts) == BLOCKS and all(len(p) == NO + NB for p in parts)
    for r in range(NO + NB):
        assert np.array_equal(np.concatenate([p[r] for p in parts]), want[r]), "slices of one block, output %d" % r
    ctx = job.configured()
    job.setup(ctx, BLENDS, GAIN, SEED)
    ctx.batch_set_sources([0, 1, 0])
    got = ctx.batch_run([job.inputs[0], job.inputs[1], None], RATE, FMT)
    ctx.close()
    for r in range(NO + NB):
        assert np.array_equal(got[r], want[r]), "source map, output %d" % r


def test_a_resumed_checkpoint_with_blends_set_again_writes_the_uninterrupted_bytes(job):
    want = job.run(FMT, gain=GAIN, dither=SEED)["outs"]
    metas = [(SAMPLES, "lpcm16", RATE)] * NCH
    cut = lambda need: [d[0][2 * f:2 * (f + c)] for d, (f, c) in zip(job.inputs, need)]
    ctx = job.configured()
    job.setup(ctx, BLENDS, GAIN, SEED)
    assert ctx.batch_stream_open(metas, RATE, FMT) == BLOCKS * BLOCK
    head = ctx.batch_stream_step(1, cut(ctx.batch_stream_need(1)))
    blob = ctx.batch_stream_checkpoint()
    ctx.batch_stream_close()
    ctx.close()
    ctx = job.configured()
    job.setup(ctx, BLENDS, GAIN, SEED)
    assert ctx.batch_stream_resume(metas, RATE, FMT, blob) == BLOCK
    tail = ctx.batch_stream_step(2, cut(ctx.batch_stream_need(2)))
    ctx.batch_stream_close()
    ctx.close()
    assert len(head) == len(tail) == NO + NB
    for r in range(NO + NB):
        assert np.array_equal(np.concatenate([head[r], tail[r]]), want[r]), "resumed: output %d" % r


def test_records_of_the_blend_ports_are_the_standalone_calls_on_the_blend_rows(job, ctx1):
    rows = job.rows()
    never = job.run("ieee64", blends=None, records=True)
    self_ref = job.run("ieee64", gain=GAIN, records=True)                   # a list of N + 3 ports: every blend port references itself
    wide = job.run("ieee64", gain=GAIN, records=True, align=[-1, 0, 0, -1, NCH, -1, -1, 0, NO + 1])      # blend 1 against channel 0, blend 2 against blend 1
    full = np.stack(rows)
    stats, bands, peaks = ctx1.block_stats(full, BLOCK), ctx1.block_spectrum(full, RATE, EDGES), ctx1.block_true_peak(full)
    for res in (self_ref, wide):
        assert res["report"].shape == (NO + NB, BLOCKS) and res["spectrum"].shape == (NO + NB, BLOCKS, len(EDGES) - 1)
        assert res["align"].shape == (NO + NB, BLOCKS) and res["true_peak"].shape == (NO + NB, BLOCKS)
        for kind in ("report", "spectrum", "align", "true_peak"):               # ports 0 .. N + 2: the run without blends
            assert res[kind][:NO].tobytes() == never[kind].tobytes(), kind
        assert res["report"][NO:].tobytes() == stats[NO:].tobytes()             # taken from s, before the gain
        assert res["spectrum"][NO:].tobytes() == bands[NO:].tobytes()
        assert res["true_peak"][NO:].tobytes() == peaks[NO:].tobytes()
    assert self_ref["align"][NO:].tobytes() == ctx1.block_align(full, [-1, 0, 0, -1, NCH, -1, NO, NO + 1, NO + 2], 64)[NO:].tobytes()
    assert wide["align"][NO:].tobytes() == ctx1.block_align(full, [-1, 0, 0, -1, NCH, -1, -1, 0, NO + 1], 64)[NO:].tobytes()
    assert wide["align"][NO + 1].tobytes() != self_ref["align"][NO + 1].tobytes()


def test_blends_taken_back_are_off(job):
    never = job.run(FMT, blends=None, dither=SEED, records=True)
    ctx = job.configured()
    job.setup(ctx, BLENDS, GAIN, SEED, records=True)
    assert ctx.batch_blends() == NB
    first = ctx.batch_run(job.inputs, RATE, FMT)                                # a call with the blends on, on this very context
    assert len(first) == NO + NB and ctx.get_option("stat_batch_device_kib") > never["kib"]
    ctx.batch_set_blends([])
    assert ctx.batch_blends() == 0
    again = ctx.batch_run(job.inputs, RATE, FMT)                                # the state has moved on: only the shape and the memory are compared
    assert len(again) == NO and ctx.get_option("stat_batch_device_kib") == never["kib"]
    assert ctx.batch_report().shape == (NO, BLOCKS)
    ctx.close()
    ctx = job.configured()
    job.setup(ctx, BLENDS, GAIN, SEED, records=True)
    ctx.batch_set_blends(None)
    back = ctx.batch_run(job.inputs, RATE, FMT)
    assert len(back) == NO and ctx.get_option("stat_batch_device_kib") == never["kib"]
    for r in range(NO):
        assert np.array_equal(back[r], never["outs"][r]), r
    assert ctx.batch_report().tobytes() == never["report"].tobytes() and ctx.batch_spectrum().tobytes() == never["spectrum"].tobytes()
    assert ctx.batch_align().tobytes() == never["align"].tobytes() and ctx.batch_true_peak().tobytes() == never["true_peak"].tobytes()
    ctx.close()


def test_a_refused_set_blends_leaves_the_next_call_unchanged(job):
    pkg = job.pkg
    want = job.run(FMT, gain=GAIN, dither=SEED)["outs"]
    ctx = job.configured()
    job.setup(ctx, BLENDS, GAIN, SEED)
    for blends, gain, what in (([[(0, 1.0)], [(3, 1.0)]], None, "blend 1, term 0"), ([[(0, 1.0), (1, float("inf"))]], None, "blend 0, term 1"),
                               ([[(0, 1.0)], []], None, "blend 1"), ([[(0, 1.0)] * 33], None, "33 terms"), ([[(0, 1.0)]], [float("nan")], "blend 0")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx.batch_set_blends(blends, gain)
        assert e.value.code == pkg.GDG_ERR_INVALID
    assert ctx.batch_blends() == NB
    metas = [(SAMPLES, "lpcm16", RATE)] * NCH
    cut = lambda need: [d[0][2 * f:2 * (f + c)] for d, (f, c) in zip(job.inputs, need)]
    assert ctx.batch_stream_open(metas, RATE, FMT) == BLOCKS * BLOCK
    with pytest.raises(pkg.GdgError, match="streamed batch run is open") as e:
        ctx.batch_set_blends([[(1, 1.0)]])
    assert e.value.code == pkg.GDG_ERR_INVALID and ctx.batch_blends() == NB
    got = ctx.batch_stream_step(BLOCKS, cut(ctx.batch_stream_need(BLOCKS)))
    ctx.batch_stream_close()
    for r in range(NO + NB):
        assert np.array_equal(got[r], want[r]), r
    # an alignment list of neither N + 3 nor N + 3 + B ports is refused when the job is described, with both numbers
    ctx.batch_align_enable([-1] * (NO + 1), 64)
    with pytest.raises(pkg.GdgError, match="%d .*%d" % (NO, NO + NB)):
        ctx.batch_run(job.inputs, RATE, FMT)
    ctx.close()
