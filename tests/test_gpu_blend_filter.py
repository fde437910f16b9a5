"""A short FIR per blend term (gdg_batch_set_blends_filtered, gdg_blend_rows_filtered) on the device, bit for bit against the numpy
restatement of the arithmetic include/gdg.h states (FILTERS; tests/blend_filter_ref.py).  The stand-alone forms: 5 rows; sample counts
shorter than the taps, odd, and crossing the tile that stops comparing against the history; tap counts {0, 1, 2, 63, 64} with delays {0, 1,
2, 4096 - 63}; blends of 1, 5 and 32 terms; with a history, without one, and on device rows offset by 8 bytes, which takes the 8-byte lanes.
The batch form: 4 channels, 6 blocks, a term whose reach spans the step before -- the blend files are the restatement of the call's own
IEEE64 chain files, and windows, slices and a source map write the same bytes.  A list without taps is the delayed call; a filter in force
refuses the checkpoint calls."""
import ctypes as C

import numpy as np
import pytest

import blend_filter_ref as ref
from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
MAXD = ref.MAX_DELAY
ROWS = 5


def taps(T, seed):
    """T taps of mixed sign and size, a zero and a negative among them"""
    h = np.random.default_rng(1000 + 7 * T + seed).uniform(-1.0, 1.0, T)
    if T > 2:
        h[T // 2] = 0.0
        h[1] *= 1e-7
    return h


# every kind of term: T in {0, 1, 2, 63, 64} with d in {0, 1, 2, 4096 - 63}, where the reach allows it (T = 64 at d = 4033 reaches 4096)
KINDS = [(T, d) for T in (0, 1, 2, 63, 64) for d in (0, 1, 2, MAXD - 63)]
assert all(d + max(T, 1) - 1 <= MAXD for T, d in KINDS) and max(d + max(T, 1) - 1 for T, d in KINDS) == MAXD


def term(i, T, d, weight=None):
    return (i % ROWS, (0.3 + 0.1 * (i % 7)) * (-1.0 if i % 3 == 0 else 1.0) if weight is None else weight, d, taps(T, i))


def lists():
    """blends of 1, 5 and 32 terms (the first and the unrolled remainders of the delayed load), over every kind; every kind also alone"""
    kinds = [term(i, T, d) for i, (T, d) in enumerate(KINDS)]
    out = [[kinds[i]] for i in range(len(kinds))]
    out.append([kinds[3], kinds[19], kinds[8], kinds[0], kinds[15]])                     # 5 terms: a tapless one first, two in the middle
    out.append([kinds[(5 * i + 2) % len(kinds)] for i in range(32)])                     # 32 terms
    out.append([kinds[16], kinds[1], kinds[2], kinds[12], kinds[3]])                     # 5 terms: 64 taps first, runs of tapless ones
    return out


LISTS = lists()


@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


def random_rows(n_rows, samples, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, (n_rows, samples))
    x[:, ::7] *= 1e-9
    return x


@pytest.fixture(scope="module")
def cases():
    """rows, history and the restatement's sums per sample count, computed once"""
    out = {}
    for samples in (10, 1501, MAXD + 513):
        x, hist = random_rows(ROWS, samples, 40 + samples), random_rows(ROWS, MAXD, 90 + samples)
        out[samples] = dict(x=x, hist=hist, want={False: ref.blends(x, LISTS, None), True: ref.blends(x, LISTS, hist)})
    return out


@pytest.mark.parametrize("samples", [10, 1501, MAXD + 513])
def test_standalone_sums_are_the_restatement(ctx1, cases, samples):
    x, hist = cases[samples]["x"], cases[samples]["hist"]
    for with_history in (False, True):
        want = cases[samples]["want"][with_history]
        got = ctx1.blend_rows_filtered(x, LISTS, hist if with_history else None)
        for b in range(len(LISTS)):
            assert ref.same_bits(got[b], want[b]), (samples, with_history, b, int(np.argmax(got[b] != want[b])))
    # device rows offset by 8 bytes: the 8-byte lanes; then the history and the sums offset in turn
    even = samples + (samples & 1)
    want = cases[samples]["want"][True]
    for off, hoff, ooff in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        d_in, d_out, d_hist = ctx1.alloc(1, ROWS * even + 2), ctx1.alloc(1, len(LISTS) * even + 2), ctx1.alloc(1, ROWS * MAXD + 2)
        padded, hp = np.full(ROWS * even + 2, 9.0), np.full(ROWS * MAXD + 2, 5.0)
        for r in range(ROWS):
            padded[off + r * even:off + r * even + samples] = x[r]
            hp[hoff + r * MAXD:hoff + (r + 1) * MAXD] = hist[r]
        d_in.upload(padded)
        d_hist.upload(hp)
        d_out.upload(np.full(d_out.cols, 7.0))
        ctx1.blend_rows_filtered_device(d_in.ptr + 8 * off, even, ROWS, samples, LISTS, d_out.ptr + 8 * ooff, even, d_hist.ptr + 8 * hoff, MAXD)
        raw = d_out.download().reshape(-1)
        for b in range(len(LISTS)):
            assert ref.same_bits(raw[ooff + b * even:ooff + b * even + samples], want[b]), (samples, off, hoff, ooff, b)
            tail = raw[ooff + b * even + samples:ooff + (b + 1) * even]
            assert np.array_equal(tail, np.full(tail.size, 7.0)), "samples outside a blend's row were written"
        assert np.array_equal(raw[:ooff], np.full(ooff, 7.0)) and np.array_equal(raw[ooff + len(LISTS) * even:], np.full(2 - ooff, 7.0))
        assert np.array_equal(d_hist.download().reshape(-1), hp) and np.array_equal(d_in.download().reshape(-1), padded)      # read, never written
        d_in.free()
        d_out.free()
        d_hist.free()


def test_known_answer_and_a_list_without_taps_is_the_delayed_call(ctx1):
    x = np.array([[0.5, -0.25, 3.0, 3.0, -0.0, 1e-300, 7.0]])
    got = ctx1.blend_rows_filtered(x, [[(0, 1.0, 0, [1.0, -1.0])]])
    assert np.array_equal(got[0], np.concatenate([x[0, :1], np.diff(x[0])])) and got[0][0] == x[0, 0] - 0.0
    assert got.tobytes() == ctx1.blend_rows_delayed(x, [[(0, 1.0, 0), (0, -1.0, 1)]]).tobytes()      # the bits of the DELAYS known answer
    # every T = 0: the bytes of gdg_blend_rows_delayed, with and without a history
    rows, hist = random_rows(3, 4099, 5), random_rows(3, MAXD, 6)
    delayed = [[(0, 0.75, 0), (1, -1.25, 1), (2, 0.5, 4096), (0, 2.0, 256)], [(1, 1.0, 2), (2, -0.3, 255), (0, 0.9, 257), (1, -1.1, 4095), (2, 0.0, 0)]]
    empty = [[t + ([],) for t in b] for b in delayed]
    for history in (None, hist):
        assert ctx1.blend_rows_filtered(rows, empty, history).tobytes() == ctx1.blend_rows_delayed(rows, delayed, history).tobytes()
        assert ctx1.blend_rows_filtered(rows, delayed, history).tobytes() == ctx1.blend_rows_delayed(rows, delayed, history).tobytes()


def test_a_nan_lands_at_exactly_the_taps_reach(ctx1):
    samples, j = 700, 300
    x = random_rows(2, samples, 11)
    x[1, j] = np.nan
    for T, d in ((1, 0), (2, 5), (63, 100), (64, 257), (0, 9)):
        got = ctx1.blend_rows_filtered(x, [[(0, 0.5, 3, taps(4, 1)), (1, -0.7, d, taps(T, 2) + 2.0)]])[0]      # taps in [1, 3]: none is zero
        first, last = j + d, j + d + max(T, 1) - 1
        want = np.zeros(samples, dtype=bool)
        want[first:last + 1] = True
        assert np.array_equal(np.isnan(got), want), (T, d)


def test_standalone_refusals_name_blend_and_term(ctx1):
    pkg = package()
    x = np.ones((2, 4))
    for blends, what in (([[(0, 1.0, 0, [1.0])], [(1, 1.0, 0, [1.0, np.nan])]], "blend 1, term 0: tap 1"), ([[(0, 1.0, 0), (1, 1.0, 0, np.ones(65))]], "blend 0, term 1 has 65 taps"),
                         ([[(0, 1.0, MAXD - 1, [1.0, 1.0, 1.0])]], "blend 0, term 0: a delay of 4095 samples and 3 taps"), ([[(0, 1.0, MAXD + 1, [1.0])]], "blend 0, term 0: delay = 4097")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx1.blend_rows_filtered(x, blends)
        assert e.value.code == pkg.GDG_ERR_INVALID


# ---- the batch form ----------------------------------------------------------------------------------------------------------------------
RATE, NCH = 48000, 4
BLOCKS = 6
SAMPLES = (BLOCKS - 1) * BLOCK + 100
NO = NCH + 3
LEVEL = 0.1
# one term of two taps, the known answer; a reach of 4000 + 64 - 1 = 4063 samples, which spans the step before at every window; the limit
# itself; five terms of every kind
BLENDS = [[(0, 1.0, 0, [1.0, -1.0])],
          [(1, 0.6, 0, taps(32, 3)), (2, 0.4, 4000, taps(64, 4))],
          [(3, 1.0, MAXD - 63, taps(64, 5))],
          [(2, -1.0, 3), (0, 0.1, 256, taps(1, 6)), (1, 0.2, 255, taps(63, 7)), (3, 0.3, 0), (0, -0.7, 4095, taps(2, 8))]]
NB = len(BLENDS)
assert max(ref.reach(t) for b in BLENDS for t in b) == MAXD and ref.reach(BLENDS[1][1]) > 4000
DELAYED = [[t[:3] for t in b] for b in BLENDS]


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """4 channels with short chains -- power amps of 300, 64, 128 and 32 taps, the third on the file of channel 0 (so the job can be described
    with a source map); 5 * 8192 + 100 samples: 6 blocks."""

    def __init__(self):
        self.pkg = package()
        files = [lpcm16_file(LEVEL * synth_signal(c, SAMPLES, RATE)) for c in range(3)]
        self.inputs = [(files[0], "lpcm16", RATE), (files[1], "lpcm16", RATE), (files[0], "lpcm16", RATE), (files[2], "lpcm16", RATE)]
        self.irs = [synth_ir(n, seed=290 + c) for c, n in enumerate((300, 64, 128, 32))]
        self.metas = [(SAMPLES, "lpcm16", RATE)] * NCH
        self.cache = {}

    def cut(self, need):
        return [d[0][2 * f:2 * (f + c)] for d, (f, c) in zip(self.inputs, need)]

    def configured(self, window=2, blends=BLENDS, report=False):
        ctx = self.pkg.Context(NCH, BLOCK)
        for c in range(NCH):
            ctx.append_unit(c, "power_amp", fir=self.irs[c])
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(NCH):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * c, 1.0 + 0.5 * c, 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
        ctx.metronome_configure(4, 150, RATE)
        ctx.set_window(window)
        if report:
            ctx.batch_report_enable()
        if blends is not None:
            ctx.batch_set_blends(blends)
        return ctx

    def run(self, blends=BLENDS, window=2, report=False):
        key = (None if blends is None else str(blends), window, report)
        if key not in self.cache:
            ctx = self.configured(window, blends, report)
            outs = ctx.batch_run(self.inputs, RATE, "ieee64")
            self.cache[key] = dict(outs=outs, kib=ctx.get_option("stat_batch_device_kib"), max_delay=ctx.batch_blend_max_delay(), max_reach=ctx.batch_blend_max_reach(),
                                   report=ctx.batch_report() if report else None)
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
    res = job.run()
    outs = res["outs"]
    assert len(outs) == NO + NB and res["max_delay"] == 4095 and res["max_reach"] == MAXD
    rows = [o.view(np.float64) for o in outs]
    assert all(r.size == BLOCKS * BLOCK for r in rows) and all(np.isfinite(r).all() and r.any() for r in rows[:NCH])
    want = ref.blends(np.stack(rows[:NCH]), BLENDS)
    for b in range(NB):
        assert ref.same_bits(rows[NO + b], want[b]), (b, int(np.argmax(rows[NO + b] != want[b])))
    assert np.array_equal(rows[NO], np.concatenate([rows[0][:1], np.diff(rows[0])]))      # the known answer
    assert not rows[NO + 2][:MAXD - 63].any() and rows[NO + 2][MAXD - 63:].any()            # zeros in front of the job
    # chain, master and metronome files are those of the job without blends
    same_files(outs[:NO], job.run(blends=None)["outs"], "without blends")


def test_windows_slices_and_a_source_map_write_the_same_bytes(job):
    want = job.run()["outs"]
    for window in (1, 4):
        same_files(job.run(window=window)["outs"], want, "window %d" % window)
    ctx = job.configured()
    assert ctx.batch_stream_open(job.metas, RATE, "ieee64") == BLOCKS * BLOCK
    parts = [ctx.batch_stream_step(n, job.cut(ctx.batch_stream_need(n))) for n in (1, 2, 3)]
    ctx.batch_stream_close()
    same_files([np.concatenate([p[r] for p in parts]) for r in range(NO + NB)], want, "slices of 1 + 2 + 3 blocks")
    second = ctx.batch_run(job.inputs, RATE, "ieee64")                          # a second job begins from zeros, not from the first one's tail
    ctx.close()
    rows = [o.view(np.float64) for o in second]
    assert ref.same_bits(rows[NO + 1], ref.blend(np.stack(rows[:NCH]), BLENDS[1])) and not rows[NO + 2][:MAXD - 63].any()
    ctx = job.configured()
    ctx.batch_set_sources([0, 1, 0, 3])
    got = ctx.batch_run([job.inputs[0], job.inputs[1], None, job.inputs[3]], RATE, "ieee64")
    ctx.close()
    same_files(got, want, "source map")


def test_a_filtered_port_s_records_are_those_of_its_file(job):
    res = job.run(report=True)
    same_files(res["outs"], job.run()["outs"], "with the report on")
    report = res["report"]
    assert report.shape == (NO + NB, BLOCKS)
    ctx = job.pkg.Context(1, BLOCK)
    for b in range(NB):
        row = res["outs"][NO + b].view(np.float64)
        own = ctx.block_stats(row, BLOCK)[0]
        assert report[NO + b].tobytes() == own.tobytes(), b
        sums = np.array([np.sum(row[q * BLOCK:(q + 1) * BLOCK] ** 2) for q in range(BLOCKS)])
        assert np.allclose(report[NO + b]["sum_sq"], sums, rtol=1e-12, atol=0.0) and sums.all(), b      # 8192 adds of positive doubles: far inside 8192 * 2^-53
    ctx.close()


def test_a_nan_in_a_chain_row_lands_where_the_taps_reach():
    """through the batch table's own layout: the setting packs gains between the weights and the taps, the stand-alone call does not -- here
    the packed list in force is read by a batch run of one silent channel whose input holds one NaN, across a step's edge"""
    pkg = package()
    ctx = pkg.Context(1, BLOCK)
    ctx.set_window(1)
    j, d, T = 4150, 4000, 64                                                   # the NaNs at 8150 .. 8213: both sides of sample 8192
    x = np.zeros(2 * BLOCK)
    x[j] = np.nan
    ctx.batch_set_blends([[(0, 1.0, d, taps(T, 9) + 2.0)], [(0, 1.0, 0, [1.0])]], gain=[0.5, 2.0])
    outs = ctx.batch_run([(np.ascontiguousarray(x).view(np.uint8), "ieee64", RATE)], RATE, "ieee64")
    ctx.close()
    at = np.flatnonzero(np.isnan(outs[0].view(np.float64)))                    # where the chain row itself has NaNs: at j at least
    assert at.size >= 1 and at[0] == j and at[-1] + d + T <= 2 * BLOCK
    want = np.zeros(2 * BLOCK, dtype=bool)
    for i in at:
        want[i + d:i + d + T] = True
    assert np.array_equal(np.isnan(outs[4].view(np.float64)), want) and want[BLOCK - 1:BLOCK + 1].all()
    assert np.array_equal(np.flatnonzero(np.isnan(outs[5].view(np.float64))), at)


def test_no_taps_is_the_delayed_call_and_a_filter_refuses_the_checkpoint_calls(job):
    pkg, lib = job.pkg, job.pkg.lib()
    # tap_first = None: the buffers and the bytes of the delayed call; so with empty tap lists
    delayed = job.run(blends=DELAYED)
    empty = job.run(blends=[[t[:3] + ([],) for t in b] for b in BLENDS])
    assert empty["kib"] == delayed["kib"] and empty["max_reach"] == delayed["max_reach"] == delayed["max_delay"] == 4095
    same_files(empty["outs"], delayed["outs"], "empty tap lists")
    first, channel, weight = pkg.Context._blend_csr(DELAYED)
    delay = pkg.Context._blend_delays(DELAYED)
    ctx = job.configured(blends=None)
    ctx._check(lib.gdg_batch_set_blends_filtered(ctx._h, NB, first.ctypes.data, channel.ctypes.data, weight.ctypes.data, delay.ctypes.data, None, None, None))
    assert ctx.batch_blend_max_reach() == 4095 and ctx.batch_blend_max_delay() == 4095
    got = ctx.batch_run(job.inputs, RATE, "ieee64")
    assert ctx.get_option("stat_batch_device_kib") == delayed["kib"]
    same_files(got, delayed["outs"], "tap_first == NULL")
    # a filter that reaches nowhere -- T = 1, d = 0 -- keeps no history; d = 0, T = 2 costs exactly the history
    ctx.batch_set_blends([[(c, w, 0) for c, w, _ in b] for b in DELAYED])
    ctx.batch_run(job.inputs, RATE, "ieee64")
    plain_kib = ctx.get_option("stat_batch_device_kib")
    ctx.batch_set_blends([[(c, w, 0, [0.5]) for c, w, _ in b] for b in DELAYED])
    ctx.batch_run(job.inputs, RATE, "ieee64")
    assert ctx.batch_blend_max_reach() == 0 and ctx.get_option("stat_batch_device_kib") == plain_kib
    ctx.batch_set_blends([[(c, w, 0, [0.5, 0.5]) for c, w, _ in b] for b in DELAYED])
    ctx.batch_run(job.inputs, RATE, "ieee64")
    assert ctx.batch_blend_max_reach() == 1 and ctx.batch_blend_max_delay() == 0
    assert ctx.get_option("stat_batch_device_kib") - plain_kib == NCH * MAXD * 8 // 1024
    ctx.close()

    # every T = 0, d = 0 through the filtered call: a checkpoint is what it was
    stateless = [[(c, w, 0, []) for c, w, _ in b] for b in DELAYED]
    ctx = job.configured(blends=stateless)
    assert ctx.batch_blend_max_reach() == 0
    assert ctx.batch_stream_open(job.metas, RATE, "ieee64") == BLOCKS * BLOCK
    head = ctx.batch_stream_step(1, job.cut(ctx.batch_stream_need(1)))
    blob = ctx.batch_stream_checkpoint()
    ctx.batch_stream_close()
    ctx.close()
    ctx = job.configured(blends=stateless)
    assert ctx.batch_stream_resume(job.metas, RATE, "ieee64", blob) == BLOCK
    tail = ctx.batch_stream_step(BLOCKS - 1, job.cut(ctx.batch_stream_need(BLOCKS - 1)))
    ctx.batch_stream_close()
    same_files([np.concatenate([head[r], tail[r]]) for r in range(NO + NB)], job.run(blends=[[(c, w, 0) for c, w, _ in b] for b in DELAYED])["outs"], "resumed")

    # d = 0, T = 2: checkpoint size, checkpoint and resume are unsupported, and nothing is written
    ctx.batch_set_blends([[(0, 1.0, 0, [1.0, -1.0])]])
    assert ctx.batch_blend_max_delay() == 0 and ctx.batch_blend_max_reach() == 1
    assert ctx.batch_stream_open(job.metas, RATE, "ieee64") == BLOCKS * BLOCK
    ctx.batch_stream_step(1, job.cut(ctx.batch_stream_need(1)))
    size, written = C.c_size_t(123), C.c_size_t(456)
    buf = C.create_string_buffer(b"\xaa" * (len(blob) + 4096), len(blob) + 4096)
    assert lib.gdg_batch_stream_checkpoint_size(ctx._h, C.byref(size)) == pkg.GDG_ERR_UNSUPPORTED and size.value == 123
    assert lib.gdg_batch_stream_checkpoint(ctx._h, buf, len(blob) + 4096, C.byref(written)) == pkg.GDG_ERR_UNSUPPORTED and written.value == 456
    assert "not in the version-1 container" in lib.gdg_last_error(ctx._h).decode() and buf.raw == b"\xaa" * (len(blob) + 4096)
    with pytest.raises(pkg.GdgError, match="streamed batch run is open"):       # and the setting cannot change under an open job
        ctx.batch_set_blends([[(0, 1.0, 0, [1.0])]])
    ctx.batch_stream_close()
    with pytest.raises(pkg.GdgError, match="blend history") as e:
        ctx.batch_stream_resume(job.metas, RATE, "ieee64", blob)
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    # the shard calls refuse blends as ever
    for call in (lambda: ctx.batch_run_shard(job.inputs, RATE, "ieee64"), lambda: ctx.batch_stream_open_shard(job.metas, RATE, "ieee64"),
                 lambda: ctx.batch_stream_resume_shard(job.metas, RATE, "ieee64", blob)):
        with pytest.raises(pkg.GdgError, match="1 blends are in force") as e:
            call()
        assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    with pytest.raises(pkg.GdgError):                                            # ... so the fourth never finds a job of theirs open
        ctx.batch_stream_step_shard(1, job.cut([(0, BLOCK)] * NCH))
    ctx.close()


def test_refusals_name_blend_and_term_and_leave_the_list_in_force(job):
    pkg = job.pkg
    want = job.run()["outs"]
    ctx = job.configured()
    for blends, what in (([[(0, 1.0, 0, [1.0])], [(1, 1.0, 0), (2, 1.0, 0, [1.0, np.inf])]], "blend 1, term 1: tap 1"),
                         ([[(0, 1.0, 0, np.ones(65))]], "blend 0, term 0 has 65 taps"),
                         ([[(0, 1.0, 1)], [(0, 1.0, MAXD - 63, np.ones(64)), (1, 1.0, MAXD - 62, np.ones(64))]], "blend 1, term 1: a delay of 4034 samples and 64 taps"),
                         ([[(0, 1.0, 5, [1.0]), (4, 1.0, 5, [1.0])]], "blend 0, term 1")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx.batch_set_blends(blends)
        assert e.value.code == pkg.GDG_ERR_INVALID
    # a tap_first that descends
    first, channel, weight = pkg.Context._blend_csr([[(0, 1.0), (1, 1.0)]])
    tap_first, tap = np.array([0, 2, 1], dtype=np.int32), np.ones(3)
    rc = pkg.lib().gdg_batch_set_blends_filtered(ctx._h, 1, first.ctypes.data, channel.ctypes.data, weight.ctypes.data, None, tap_first.ctypes.data, tap.ctypes.data, None)
    assert rc == pkg.GDG_ERR_INVALID and "blend 0, term 1: tap_first" in pkg.lib().gdg_last_error(ctx._h).decode()
    assert ctx.batch_blends() == NB and ctx.batch_blend_max_reach() == MAXD and ctx.batch_blend_max_delay() == 4095
    same_files(ctx.batch_run(job.inputs, RATE, "ieee64"), want, "after the refusals")
    ctx.close()
