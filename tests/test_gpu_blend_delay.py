"""A delay per blend term (gdg_batch_set_blends_delayed, gdg_blend_rows_delayed) on the device, bit for bit against the numpy restatement
of the arithmetic include/gdg.h states (tests/blend_delay_ref.py).  The stand-alone forms: every sample count at which a lane's or a tile's
path changes, odd and even delays, a tile edge and the maximum, with and without a history, on bases and strides that allow 16-byte lanes
and on such that do not, with infinities and NaNs planted.  The batch form at the smallest shape that crosses every boundary: 3 channels, 4
blocks, delays {0, 1, 4096, an 8-term mix} -- the blend files are the restatement of the call's own IEEE64 chain files, and windows, slices
and a source map write the same bytes: the history carries from step to step and from slice to slice, and a second job begins from zeros.
All-zero delays are gdg_batch_set_blends; a delay in force refuses the checkpoint calls and costs exactly the history's bytes."""
import ctypes as C

import numpy as np
import pytest

import blend_delay_ref as ref
import trim_ref
from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
MAXD = ref.MAX_DELAY
RATE, NCH = 48000, 3
SAMPLES, BLOCKS = 3 * BLOCK + 100, 4
NO = NCH + 3
LEVEL = 0.1
# delays 0 and 1, the maximum, and 8 terms over every kind of delay (the unrolled four and the rest, a channel named three times)
BLENDS = [[(0, 1.0, 0)], [(0, 1.0, 0), (0, -1.0, 1)], [(1, 0.6, 0), (2, 0.4, 4096)],
          [(2, -1.0, 3), (0, 0.1, 256), (1, 0.2, 255), (2, 0.3, 0), (0, -0.7, 4095), (1, 0.5, 2), (2, 0.25, 257), (0, 1.5, 1000)]]
NB = len(BLENDS)
PLAIN = [[(c, w) for c, w, _ in b] for b in BLENDS]
# the stand-alone lists: three rows, two blends, every delay of {0, 1, 2, 255, 256, 257, 4095, 4096}
LISTS = [[(0, 0.75, 0), (1, -1.25, 1), (2, 0.5, 4096), (0, 2.0, 256)], [(1, 1.0, 2), (2, -0.3, 255), (0, 0.9, 257), (1, -1.1, 4095), (2, 0.0, 0)]]


# ---- the stand-alone forms ---------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("samples", [1, 3, 5, 4095, 4096, 4097, 8193])
def test_standalone_sums_are_the_restatement(ctx1, samples):
    x = random_rows(3, samples, 300 + samples)
    x[2, samples // 2] = np.inf                                             # under the zero weight of the last term: 0 * inf is NaN
    hist = random_rows(3, MAXD, 900 + samples)
    for history in (None, hist):
        want = ref.blends(x, LISTS, history)
        assert np.isnan(want[1][samples // 2])
        got = ctx1.blend_rows_delayed(x, LISTS, history)
        for b in range(len(LISTS)):
            assert ref.same_bits(got[b], want[b]), (samples, history is not None, b)
        # the device form: bases and strides that allow the 16-byte form, and the same offset by one sample -- rows, history and sums in turn
        even = samples + (samples & 1)
        for stride, out_stride, hist_stride, off, hoff, ooff in ((even, even, MAXD, 0, 0, 0), (even, even, MAXD, 1, 0, 0), (even, even, MAXD, 0, 1, 0),
                                                                 (even, even, MAXD, 0, 0, 1), (even + 1, even, MAXD, 0, 0, 0), (even, even + 1, MAXD + 1, 1, 1, 1)):
            if history is None and (hoff or hist_stride != MAXD):
                continue
            d_in, d_out, d_hist = ctx1.alloc(1, 3 * stride + 2), ctx1.alloc(1, len(LISTS) * out_stride + 2), ctx1.alloc(1, 3 * hist_stride + 2)
            padded = np.full(3 * stride + 2, 9.0)
            for r in range(3):
                padded[off + r * stride:off + r * stride + samples] = x[r]
            d_in.upload(padded)
            hp = np.full(3 * hist_stride + 2, 5.0)
            if history is not None:
                for r in range(3):
                    hp[hoff + r * hist_stride:hoff + r * hist_stride + MAXD] = history[r]
            d_hist.upload(hp)
            d_out.upload(np.full(d_out.cols, 7.0))
            ctx1.blend_rows_delayed_device(d_in.ptr + 8 * off, stride, 3, samples, LISTS, d_out.ptr + 8 * ooff, out_stride,
                                           None if history is None else d_hist.ptr + 8 * hoff, hist_stride)
            raw = d_out.download().reshape(-1)
            case = (samples, history is not None, stride, out_stride, hist_stride, off, hoff, ooff)
            for b in range(len(LISTS)):
                assert ref.same_bits(raw[ooff + b * out_stride:ooff + b * out_stride + samples], want[b]), case + (b,)
                tail = raw[ooff + b * out_stride + samples:ooff + (b + 1) * out_stride]
                assert np.array_equal(tail, np.full(tail.size, 7.0)), "samples outside a blend's row were written"
            assert np.array_equal(raw[:ooff], np.full(ooff, 7.0)) and np.array_equal(raw[ooff + len(LISTS) * out_stride:], np.full(2 - ooff, 7.0))
            assert ref.same_bits(d_hist.download().reshape(-1), hp) and ref.same_bits(d_in.download().reshape(-1), padded)      # read, never written
            d_in.free()
            d_out.free()
            d_hist.free()


def test_known_answer_the_first_difference(ctx1):
    x = np.array([[0.5, -0.25, 3.0, 3.0, -0.0, 1e-300, 7.0]])
    got = ctx1.blend_rows_delayed(x, [[(0, 1.0, 0), (0, -1.0, 1)]])
    assert np.array_equal(got[0], np.concatenate([x[0, :1], np.diff(x[0])])) and got[0][0] == x[0, 0] - 0.0
    # terms without a delay through the delayed call: the stateless blend
    assert np.array_equal(ctx1.blend_rows_delayed(np.ones((3, 5)), [[(0, 0.1), (1, 0.2), (2, 0.3)]])[0], np.full(5, 0.6000000000000001))


def test_standalone_refusals_name_blend_and_term(ctx1):
    pkg = package()
    x = np.ones((2, 4))
    for lists, what in (([[(0, 1.0, 0)], [(1, 1.0, 0), (0, 1.0, MAXD + 1)]], "blend 1, term 1: delay = 4097"), ([[(0, 1.0, -1)]], "blend 0, term 0: delay = -1"),
                        ([[(0, 1.0, 1), (2, 1.0, 1)]], "blend 0, term 1"), ([[(0, 1.0, 1)], []], "blend 1 has no term")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx1.blend_rows_delayed(x, lists)
        assert e.value.code == pkg.GDG_ERR_INVALID


# ---- the batch form ----------------------------------------------------------------------------------------------------------------------
def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """3 channels with short chains -- power amps of 300, 64 and 128 taps, the third on the file of channel 0 (so the job can be described
    with a source map); 3 * 8192 + 100 samples: 4 blocks."""

    def __init__(self):
        self.pkg = package()
        files = [lpcm16_file(LEVEL * synth_signal(c, SAMPLES, RATE)) for c in range(2)]
        self.inputs = [(files[0], "lpcm16", RATE), (files[1], "lpcm16", RATE), (files[0], "lpcm16", RATE)]
        self.irs = [synth_ir(n, seed=190 + c) for c, n in enumerate((300, 64, 128))]
        self.metas = [(SAMPLES, "lpcm16", RATE)] * NCH
        self.cache = {}

    def cut(self, need):
        return [d[0][2 * f:2 * (f + c)] for d, (f, c) in zip(self.inputs, need)]

    def configured(self, window=2, blends=BLENDS):
        ctx = self.pkg.Context(NCH, BLOCK)
        for c in range(NCH):
            ctx.append_unit(c, "power_amp", fir=self.irs[c])
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(NCH):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * c, 1.0 + 0.5 * c, 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
        ctx.metronome_configure(4, 150, RATE)
        ctx.set_window(window)
        if blends is not None:
            ctx.batch_set_blends(blends)
        return ctx

    def run(self, fmt, blends=BLENDS, window=2):
        key = (fmt, None if blends is None else str(blends), window)
        if key not in self.cache:
            ctx = self.configured(window, blends)
            outs = ctx.batch_run(self.inputs, RATE, fmt)
            self.cache[key] = dict(outs=outs, kib=ctx.get_option("stat_batch_device_kib"), max_delay=ctx.batch_blend_max_delay())
            ctx.close()
        return self.cache[key]


@pytest.fixture(scope="module")
def job():
    return Job()


def same_files(got, want, what):
    assert len(got) == len(want), what
    for r in range(len(want)):
        assert np.array_equal(got[r], want[r]), "%s, output %d: %d bytes differ" % (what, r, np.count_nonzero(got[r] != want[r]))


def test_blend_files_are_the_restatement_of_the_call_s_own_chain_files(job):
    outs = job.run("ieee64")["outs"]
    assert len(outs) == NO + NB and job.run("ieee64")["max_delay"] == 4096
    rows = [o.view(np.float64) for o in outs]
    assert all(r.size == BLOCKS * BLOCK for r in rows) and all(np.isfinite(r).all() and r.any() for r in rows[:NCH])
    want = ref.blends(np.stack(rows[:NCH]), BLENDS)
    for b in range(NB):
        assert ref.same_bits(rows[NO + b], want[b]), b
    assert np.array_equal(rows[NO], rows[0])                                    # one term, no delay
    assert np.array_equal(rows[NO + 1], np.concatenate([rows[0][:1], np.diff(rows[0])]))      # the known answer
    assert np.array_equal(rows[NO + 2][:MAXD], np.float64(0.6) * rows[1][:MAXD]) and not np.array_equal(rows[NO + 2], np.float64(0.6) * rows[1])
    # lpcm24: the reference encoder on the same rows
    enc = job.run("lpcm24")["outs"]
    for b in range(NB):
        assert np.array_equal(enc[NO + b], trim_ref.encode("lpcm24", want[b], 1.0, None, NO + b, 0)), b
    # ports 0 .. N + 2 are those of the job without blends
    for fmt in ("ieee64", "lpcm24"):
        same_files(job.run(fmt)["outs"][:NO], job.run(fmt, blends=None)["outs"], "%s without blends" % fmt)


@pytest.mark.parametrize("fmt", ["ieee64", "lpcm24"])
def test_windows_slices_and_a_source_map_write_the_same_bytes(job, fmt):
    want = job.run(fmt)["outs"]
    for window in (1, 4):
        same_files(job.run(fmt, window=window)["outs"], want, "window %d" % window)
    for per in (1, 2):
        ctx = job.configured()
        parts = list(ctx.batch_stream(job.inputs, RATE, fmt, per))
        ctx.close()
        assert len(parts) == BLOCKS // per and all(len(p) == NO + NB for p in parts)
        same_files([np.concatenate([p[r] for p in parts]) for r in range(NO + NB)], want, "slices of %d" % per)
    ctx = job.configured()
    ctx.batch_set_sources([0, 1, 0])
    got = ctx.batch_run([job.inputs[0], job.inputs[1], None], RATE, fmt)
    ctx.close()
    same_files(got, want, "source map")


def test_a_second_job_on_the_context_starts_from_zero_history(job):
    """the blend ports depend on the chain rows alone, and those of a second job continue from the first job's state: so both calls' blend
    files are held against the restatement of their OWN chain files -- with zeros, not the first job's tail, in front of sample 0"""
    ctx = job.configured()
    first = ctx.batch_run(job.inputs, RATE, "ieee64")
    second = ctx.batch_run(job.inputs, RATE, "ieee64")
    parts = list(ctx.batch_stream(job.inputs, RATE, "ieee64", 3))              # and a streamed job behind them: 3 blocks, then 1
    ctx.close()
    third = [np.concatenate([p[r] for p in parts]) for r in range(NO + NB)]
    same_files(first, job.run("ieee64")["outs"], "the first job")
    for name, outs in (("second", second), ("third", third)):
        rows = [o.view(np.float64) for o in outs]
        want = ref.blends(np.stack(rows[:NCH]), BLENDS)
        for b in range(NB):
            assert ref.same_bits(rows[NO + b], want[b]), (name, b)
        assert rows[NO + 2][:MAXD].any() and np.array_equal(rows[NO + 2][:MAXD], np.float64(0.6) * rows[1][:MAXD]), name


def test_refusals_name_blend_and_term_and_leave_the_list_in_force(job):
    pkg = job.pkg
    want = job.run("lpcm24")["outs"]
    ctx = job.configured()
    for blends, what in (([[(0, 1.0, 0)], [(1, 1.0, 0), (2, 1.0, MAXD + 1)]], "blend 1, term 1: delay = 4097"), ([[(0, 1.0, -1)]], "blend 0, term 0: delay = -1"),
                         ([[(0, 1.0, 5), (3, 1.0, 5)]], "blend 0, term 1"), ([[(0, 1.0, 5)], []], "blend 1")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx.batch_set_blends(blends)
        assert e.value.code == pkg.GDG_ERR_INVALID
    assert ctx.batch_blends() == NB and ctx.batch_blend_max_delay() == 4096
    assert ctx.batch_stream_open(job.metas, RATE, "lpcm24") == BLOCKS * BLOCK
    with pytest.raises(pkg.GdgError, match="streamed batch run is open"):
        ctx.batch_set_blends([[(1, 1.0, 7)]])
    got = ctx.batch_stream_step(BLOCKS, job.cut(ctx.batch_stream_need(BLOCKS)))
    ctx.batch_stream_close()
    ctx.close()
    same_files(got, want, "after the refusals")


def test_all_zero_delays_are_the_blends_without_delays(job):
    plain = job.run("lpcm24", blends=PLAIN)
    zeros = job.run("lpcm24", blends=[[(c, w, 0) for c, w in b] for b in PLAIN])
    assert zeros["max_delay"] == 0 and plain["max_delay"] == 0 and zeros["kib"] == plain["kib"]
    same_files(zeros["outs"], plain["outs"], "all-zero delays")
    assert not np.array_equal(plain["outs"][NO + 1], job.run("lpcm24")["outs"][NO + 1])
    # a checkpoint is what it was: cut after one block, resumed in a fresh context
    ctx = job.configured(blends=[[(c, w, 0) for c, w in b] for b in PLAIN])
    assert ctx.batch_stream_open(job.metas, RATE, "lpcm24") == BLOCKS * BLOCK
    head = ctx.batch_stream_step(1, job.cut(ctx.batch_stream_need(1)))
    blob = ctx.batch_stream_checkpoint()
    ctx.batch_stream_close()
    ctx.close()
    ctx = job.configured(blends=[[(c, w, 0) for c, w in b] for b in PLAIN])
    assert ctx.batch_stream_resume(job.metas, RATE, "lpcm24", blob) == BLOCK
    tail = ctx.batch_stream_step(BLOCKS - 1, job.cut(ctx.batch_stream_need(BLOCKS - 1)))
    ctx.batch_stream_close()
    ctx.close()
    same_files([np.concatenate([head[r], tail[r]]) for r in range(NO + NB)], plain["outs"], "resumed")


def test_a_delay_in_force_refuses_the_checkpoint_calls_and_costs_the_history(job):
    pkg, lib = job.pkg, job.pkg.lib()
    plain, delayed, never = job.run("lpcm24", blends=PLAIN), job.run("lpcm24"), job.run("lpcm24", blends=None)
    assert delayed["kib"] - plain["kib"] == NCH * MAXD * 8 // 1024               # exactly the history: N x 4096 doubles
    kib = lambda: ctx.get_option("stat_batch_device_kib")
    ctx = job.configured(blends=PLAIN)
    assert ctx.batch_stream_open(job.metas, RATE, "lpcm24") == BLOCKS * BLOCK
    ctx.batch_stream_step(1, job.cut(ctx.batch_stream_need(1)))
    blob = ctx.batch_stream_checkpoint()                                         # without delays: a checkpoint to resume from below
    ctx.batch_stream_close()
    ctx.batch_run(job.inputs, RATE, "lpcm24")                                    # the buffers at the whole job's size, as in `plain`
    assert kib() == plain["kib"]
    ctx.batch_set_blends(BLENDS)
    assert ctx.batch_blend_max_delay() == 4096 and kib() == plain["kib"]         # the history comes with the first job that needs it
    ctx.batch_run(job.inputs, RATE, "lpcm24")
    assert kib() == delayed["kib"]
    assert ctx.batch_stream_open(job.metas, RATE, "lpcm24") == BLOCKS * BLOCK
    ctx.batch_stream_step(1, job.cut(ctx.batch_stream_need(1)))
    size, written = C.c_size_t(123), C.c_size_t(456)
    buf = C.create_string_buffer(b"\xaa" * (len(blob) + 4096), len(blob) + 4096)
    assert lib.gdg_batch_stream_checkpoint_size(ctx._h, C.byref(size)) == pkg.GDG_ERR_UNSUPPORTED and size.value == 123
    assert "not in the version-1 container" in lib.gdg_last_error(ctx._h).decode()
    assert lib.gdg_batch_stream_checkpoint(ctx._h, buf, len(blob) + 4096, C.byref(written)) == pkg.GDG_ERR_UNSUPPORTED and written.value == 456
    assert "not in the version-1 container" in lib.gdg_last_error(ctx._h).decode() and buf.raw == b"\xaa" * (len(blob) + 4096)
    with pytest.raises(pkg.GdgError, match="blend history") as e:
        ctx.batch_stream_checkpoint()
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    ctx.batch_stream_close()
    with pytest.raises(pkg.GdgError, match="blend history") as e:              # a resume: refused, and no job is open afterwards
        ctx.batch_stream_resume(job.metas, RATE, "lpcm24", blob)
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    with pytest.raises(pkg.GdgError, match="no streamed batch run is open"):
        ctx.batch_stream_close()
    # the delays taken back: the history goes at once, and the checkpoint calls work again
    ctx.batch_set_blends(PLAIN)
    assert ctx.batch_blend_max_delay() == 0 and kib() == plain["kib"]
    assert ctx.batch_stream_resume(job.metas, RATE, "lpcm24", blob) == BLOCK
    assert len(ctx.batch_stream_checkpoint()) == len(blob)
    ctx.batch_stream_close()
    ctx.batch_set_blends(BLENDS)
    ctx.batch_run(job.inputs, RATE, "lpcm24")
    assert kib() == delayed["kib"]
    ctx.batch_set_blends([])                                                     # the blends off: the history goes with them
    ctx.batch_run(job.inputs, RATE, "lpcm24")
    assert kib() == never["kib"]
    ctx.close()
