"""The ratio stage of the delivery (include/gdg.h, DELIVERY, "a rational ratio behind the factor") on the device, bit for bit against the numpy
restatement (tests/deliver_ratio_ref.py) run with the library's own table: the stand-alone kernel at every size and first index at which it
takes another path, with and without a history, on the 16-byte and the 8-byte load path, with sentinels around what it may write; the known
answers; a stream continued through the history; a batch job whose every port equals the restatement of its session-rate row however the job
is cut, through the plain and the dithered encoders; the records, which stay those of the render; off; and what is refused."""
import numpy as np
import pytest

import deliver_ref
import deliver_ratio_ref as ref
import dither_ref
from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
RATIOS = [(147, 160), (160, 147), (2, 3), (3, 2), (1, 2), (2, 1)]
TAP_SUM_SPREAD = 3e-6                                                       # the tap sums lie within 3e-6 of 1 (include/gdg.h; DESIGN.md 4.12j records 2.98e-6)


@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def tables():
    return {r: package().deliver_ratio_taps(*r) for r in RATIOS}


def tile_span(up, down):
    """one more intermediate sample than 256 outputs span"""
    return 256 * down // up + 1


# ---- 1: the stand-alone stage --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", RATIOS)
def test_known_answers(ctx1, tables, ratio):
    up, down = ratio
    tap = tables[ratio]
    T = tap.shape[1]
    assert T == ref.tap_count(up, down)
    g = tap.T.reshape(-1)                                                    # g[p + t L] = tap[p][t]
    samples = 4 * T
    n_out = ref.count(0, samples, up, down)
    for at in (0, 1):
        x = np.zeros(samples)
        x[at] = 1.0
        got = ctx1.deliver_rows_ratio(x, up, down)
        want = np.array([g[n * down - at * up] if 0 <= n * down - at * up < g.size else 0.0 for n in range(n_out)])
        assert got.size == n_out and np.array_equal(got, want), (ratio, at)
        assert not np.signbit(got[want == 0.0]).any()                       # +0.0 after the prototype's end (and in front of an impulse at 1)
    y = ctx1.deliver_rows_ratio(np.zeros(samples), up, down)
    assert not y.any() and not np.signbit(y).any()                          # silence: exactly +0.0
    y = ctx1.deliver_rows_ratio(np.ones(samples), up, down)
    settled = y[ref.first_out(T, up, down):]                                 # outputs whose T samples are all 1.0
    assert settled.size and float(np.abs(settled - 1.0).max()) <= TAP_SUM_SPREAD, (ratio, float(np.abs(settled - 1.0).max()))


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("n_rows", [1, 3])
def test_rows_against_the_restatement_with_sentinels(ctx1, tables, ratio, n_rows):
    up, down = ratio
    tap = tables[ratio]
    T = tap.shape[1]
    rng = np.random.default_rng(1000 * up + down + n_rows)
    sizes = [1, 2, T - 1, T, 255, 256, 257, tile_span(up, down), 3001]
    firsts = [0, 1, down - 1, down, (1 << 32) + 12345]
    case = 0
    for samples in sizes:
        for first in (firsts if samples in (1, 257, 3001) else firsts[case % 5:case % 5 + 1]):
            case += 1
            n_out = ref.count(first, samples, up, down)
            with_history = bool(case & 1)
            odd = bool(case & 2)                                             # an odd stride and a base 8 bytes off a 16-byte boundary: the 8-byte loads
            stride, out_stride = ((samples + 8) | 1) if odd else ((samples + 9) & ~1), n_out + 5
            skew = 1 if odd else 0
            x = rng.uniform(-1.0, 1.0, (n_rows, samples))
            hist = rng.uniform(-1.0, 1.0, (n_rows, ref.HISTORY)) if with_history else None
            d_in, d_out, d_hist = ctx1.alloc(1, n_rows * stride + 2), ctx1.alloc(n_rows, out_stride), ctx1.alloc(n_rows, ref.HISTORY)
            padded = np.full(n_rows * stride + 2, np.nan)
            for r in range(n_rows):
                padded[skew + r * stride:skew + r * stride + samples] = x[r]
            d_in.upload(padded.reshape(1, -1))
            d_out.upload(np.full((n_rows, out_stride), np.nan))
            if with_history:
                d_hist.upload(hist)
            ctx1.deliver_rows_ratio_device(d_in.ptr + 8 * skew, stride, n_rows, samples, up, down, first, d_hist.ptr if with_history else None, d_out.ptr, out_stride)
            got, after = d_out.download(), d_hist.download()
            for b in (d_in, d_out, d_hist):
                b.free()
            want = ref.deliver(x, up, down, first, hist, tap)
            assert want.shape == (n_rows, n_out)
            assert np.array_equal(got[:, :n_out], want), (ratio, n_rows, samples, first, with_history, odd)
            assert np.isnan(got[:, n_out:]).all(), "samples behind the produced outputs were written"
            if with_history:
                assert np.array_equal(after, ref.next_history(x, hist)), (ratio, n_rows, samples)
            h2 = None if hist is None else hist.copy()                       # the host form, compact rows
            assert np.array_equal(ctx1.deliver_rows_ratio(x, up, down, first, h2), want), (ratio, samples, first)
            if with_history:
                assert np.array_equal(h2, ref.next_history(x, hist))


@pytest.mark.parametrize("ratio", [(147, 160), (160, 147), (1, 2)])
def test_a_row_cut_anywhere_is_the_row_in_one_call(ctx1, tables, ratio):
    up, down = ratio
    x = np.random.default_rng(up + down).uniform(-1.0, 1.0, (2, 5003))
    whole = ctx1.deliver_rows_ratio(x, up, down)
    assert np.array_equal(whole, ref.deliver(x, up, down, 0, None, tables[ratio]))
    for cut in (1, 126, 127, 128, 1000):
        hist = np.zeros((2, ref.HISTORY))
        parts, first = [], 0
        while first < x.shape[1]:
            n = min(cut, x.shape[1] - first) if first == 0 or cut >= 126 else x.shape[1] - first      # a cut of 1: one sample, then the rest
            parts.append(ctx1.deliver_rows_ratio(x[:, first:first + n], up, down, first, hist))
            first += n
        assert np.array_equal(np.concatenate(parts, axis=1), whole), (ratio, cut)
    assert np.array_equal(ctx1.deliver_rows_ratio(x, 1, 1), x)               # 1/1 copies


def test_standalone_refusals(ctx1):
    pkg = package()
    for up, down, text in ((294, 320, "delivery ratio 294/320 is not reduced; pass 147/160"), (4, 2, "delivery ratio 4/2 is not reduced; pass 2/1"), (1, 3, "delivery ratio 1/3"),
                           (3, 1, "delivery ratio 3/1"), (161, 160, "delivery ratio 161/160"), (0, 1, "delivery ratio 0/1"), (147, 320, "delivery ratio 147/320")):
        with pytest.raises(pkg.GdgError, match=text) as e:
            ctx1.deliver_rows_ratio(np.zeros(16), up, down)
        assert e.value.code == pkg.GDG_ERR_INVALID
    x, out = np.zeros(160), np.zeros(10)
    rc = pkg.lib().gdg_out_ratio_rows(ctx1._h, x.ctypes.data, 1, 160, 147, 160, 0, None, out.ctypes.data, 10)      # 147 outputs do not fit
    assert rc == pkg.GDG_ERR_INVALID and "delivery ratio 147/160" in pkg.lib().gdg_last_error(ctx1._h).decode()
    assert ctx1.deliver_rows_ratio(np.zeros(160), 147, 160).size == 147     # the context is usable afterwards


# ---- 2: the batch job ----------------------------------------------------------------------------------------------------------------------
NCH, BLOCKS, SEED = 2, 3, 0x51c7e9a30b2d4f68
LEVEL = 0.1
KW = dict(metronome_to_master=True)
BLENDS = [[(0, 0.6), (1, -0.4)]]
BLEND_GAIN = [0.8]
TRIM = np.array([0.5, -1.0, 0.9, -0.7, 1.5])
NP = NCH + 3 + len(BLENDS)
PORTS = list(range(NCH)) + [dither_ref.PORT_LEFT, dither_ref.PORT_RIGHT, dither_ref.PORT_METRONOME, NCH + 3]
COMBOS = [(1, 147, 160, 48000), (2, 147, 160, 96000)]


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """2 channels, a one-unit chain each; 2 * 8192 + 1000 samples: 3 blocks; metronome to master; one two-term blend."""

    def __init__(self, rate):
        self.pkg = package()
        self.rate = rate
        samples = 2 * BLOCK + 1000
        self.inputs = [(lpcm16_file(LEVEL * synth_signal(c, samples, rate)), "lpcm16", rate) for c in range(NCH)]
        self.metas = [(samples, "lpcm16", rate)] * NCH
        self.cache = {}

    def configured(self, window=2, delivery=None, shaped=False, records=False):
        ctx = self.pkg.Context(NCH, BLOCK)
        ctx.append_unit(0, "overdrive", params=[0, 20, 100, 0, 1, 2])
        ctx.append_unit(1, "tone_stack")
        ctx.spatializer_set_sample_rate(self.rate)
        for c in range(NCH):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * c, 1.0 + 0.5 * c, 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
        ctx.metronome_configure(4, 150, self.rate)
        ctx.set_window(window)
        ctx.batch_set_blends(BLENDS, BLEND_GAIN if shaped else None)
        if shaped:
            ctx.batch_set_dither(1, SEED, 0)
            ctx.batch_set_trim(TRIM[:NCH], *TRIM[NCH:])
        if records:
            ctx.batch_report_enable()
            ctx.batch_true_peak_enable()
            ctx.meter_configure(2 * NCH + 3)                                 # inputs | outputs | metronome | left, right
            ctx.meter_set_enabled(True)
        if delivery is not None:
            ctx.batch_set_delivery_ratio(*delivery)
        return ctx

    def run(self, fmt, delivery=None, shaped=False, records=False, run_meters=False):
        key = (fmt, delivery, shaped, records, run_meters)
        if key not in self.cache:
            ctx = self.configured(delivery=delivery, shaped=shaped, records=records)
            outs = ctx.batch_run(self.inputs, self.rate, fmt, run_meters=run_meters, **KW)
            res = dict(outs=outs, kib=ctx.get_option("stat_batch_device_kib"), up=ctx.get_option("stat_batch_upload_bytes"))
            if records:
                res.update(report=ctx.batch_report().tobytes(), true_peak=ctx.batch_true_peak().tobytes())
            if run_meters:
                res.update(meters=repr([ctx.meter_state(p) for p in range(2 * NCH + 3)]))
            ctx.close()
            self.cache[key] = res
        return self.cache[key]

    def delivered(self, factor, up, down):
        """the restatement applied to the float64 rows of the same job without delivery (an IEEE64 render, whose bytes ARE the rows)"""
        key = ("want", factor, up, down)
        if key not in self.cache:
            rows = [o.view(np.float64) for o in self.run("ieee64")["outs"]]
            assert len(rows) == NP and all(r.size == BLOCKS * BLOCK and r.any() for r in rows)
            tap = self.pkg.deliver_ratio_taps(up, down)
            self.cache[key] = [ref.deliver(deliver_ref.deliver(r, factor), up, down, 0, None, tap) for r in rows]
        return self.cache[key]


@pytest.fixture(scope="module")
def jobs():
    return {rate: Job(rate) for rate in (48000, 96000)}


@pytest.mark.parametrize("combo", COMBOS)
def test_every_port_is_the_restatement_of_its_row(jobs, combo):
    factor, up, down, rate = combo
    job = jobs[rate]
    want = job.delivered(factor, up, down)
    n = ref.delivered_samples(factor, up, down, 0, BLOCKS * BLOCK)
    assert n == job.pkg.batch_delivery_samples(factor, up, down, 0, BLOCKS * BLOCK) == want[0].size
    outs = job.run("ieee64", (factor, up, down))["outs"]
    enc = job.configured(window=1)
    gains = list(TRIM) + BLEND_GAIN
    for r in range(NP):
        got = outs[r].view(np.float64)
        assert got.size == n and np.array_equal(got, want[r]), "%r, port %d: %d samples differ" % (combo, r, np.count_nonzero(got != want[r]))
    for fmt in ("lpcm16", "lpcm24"):
        plain = job.run(fmt, (factor, up, down))["outs"]
        shaped = job.run(fmt, (factor, up, down), shaped=True)["outs"]
        for r in range(NP):
            assert np.array_equal(plain[r], enc.wave_encode(fmt, want[r])), (combo, fmt, r)
            # dither, trim and blend gain on: sample n of the delivered row has the index n of the delivered job
            assert np.array_equal(shaped[r], enc.wave_encode_trim(fmt, want[r], gains[r], 1, SEED, PORTS[r], 0)), (combo, fmt, r)
        assert not np.array_equal(plain[0], shaped[0])
    enc.close()


@pytest.mark.parametrize("combo", COMBOS)
def test_every_cut_writes_the_same_bytes(jobs, combo):
    factor, up, down, rate = combo
    job = jobs[rate]
    want = job.run("lpcm24", (factor, up, down), shaped=True)["outs"]
    for window, slices in ((1, None), (2, None), (2, [1, 2]), (1, [2, 1])):
        ctx = job.configured(window=window, delivery=(factor, up, down), shaped=True)
        if slices is None:
            got = ctx.batch_run(job.inputs, rate, "lpcm24", **KW)
        else:
            left = list(slices)
            pieces = list(ctx.batch_stream(job.inputs, rate, "lpcm24", lambda _left: left.pop(0), **KW))
            done = [sum(slices[:i]) * BLOCK for i in range(len(slices))]
            assert [p[0].size for p in pieces] == [3 * job.pkg.batch_delivery_samples(factor, up, down, d, b * BLOCK) for d, b in zip(done, slices)]
            got = [np.concatenate([p[r] for p in pieces]) for r in range(NP)]
        ctx.close()
        for r in range(NP):
            assert np.array_equal(got[r], want[r]), (combo, window, slices, r)


def test_records_and_meters_are_those_of_the_render(jobs):
    job = jobs[48000]
    never = job.run("lpcm16", records=True, run_meters=True)
    with_it = job.run("lpcm16", (1, 147, 160), records=True, run_meters=True)
    for kind in ("report", "true_peak", "meters"):
        assert with_it[kind] == never[kind], kind
    assert with_it["outs"][0].size == 2 * ref.delivered_samples(1, 147, 160, 0, BLOCKS * BLOCK)


def test_off_is_off(jobs):
    job = jobs[48000]
    never = job.run("lpcm24", shaped=True)
    one = job.run("lpcm24", (1, 1, 1), shaped=True)
    ctx = job.configured(shaped=True)
    ctx.batch_set_delivery(1)
    plain_one = ctx.batch_run(job.inputs, 48000, "lpcm24", **KW)
    assert ctx.get_option("stat_batch_upload_bytes") == never["up"] and ctx.get_option("stat_batch_device_kib") == never["kib"]
    ctx.close()
    for r in range(NP):
        assert np.array_equal(one["outs"][r], never["outs"][r]) and np.array_equal(plain_one[r], never["outs"][r]), r
    assert one["kib"] == never["kib"] > 0 and one["up"] == never["up"]
    ctx = job.configured(shaped=True)
    ctx.batch_set_delivery(4)
    assert ctx.batch_delivery_ratio() == (1, 1)
    a = ctx.batch_run(job.inputs, 48000, "lpcm24", **KW)
    ctx.close()
    b = job.run("lpcm24", (4, 1, 1), shaped=True)["outs"]
    for r in range(NP):
        assert np.array_equal(a[r], b[r]) and a[r].size * 4 == never["outs"][r].size, r
    # a ratio set and taken back: the buffers go, and the bytes are those of the second job of a context that never heard of the call
    ctx = job.configured(delivery=(1, 147, 160), shaped=True)
    ctx.batch_run(job.inputs, 48000, "lpcm24", **KW)
    ctx.batch_set_delivery_ratio(1, 1, 1)
    back = ctx.batch_run(job.inputs, 48000, "lpcm24", **KW)
    plain = job.configured(shaped=True)
    plain.batch_run(job.inputs, 48000, "lpcm24", **KW)
    second = plain.batch_run(job.inputs, 48000, "lpcm24", **KW)
    for r in range(NP):
        assert np.array_equal(back[r], second[r]), r
    assert ctx.get_option("stat_batch_device_kib") == plain.get_option("stat_batch_device_kib") == never["kib"]
    ctx.close()
    plain.close()


def test_refusals_name_the_ratio_and_leave_the_context_usable(jobs):
    job = jobs[48000]
    pkg = job.pkg
    ctx = job.configured(delivery=(1, 147, 160))
    ctx.batch_set_blends(None)
    for args, text in (((1, 294, 320), "delivery ratio 294/320 is not reduced; pass 147/160"), ((1, 1, 3), "delivery ratio 1/3"), ((3, 147, 160), "delivery factor 3")):
        with pytest.raises(pkg.GdgError, match=text) as e:
            ctx.batch_set_delivery_ratio(*args)
        assert e.value.code == pkg.GDG_ERR_INVALID and (ctx.batch_delivery(), ctx.batch_delivery_ratio()) == (1, (147, 160))
    half = np.zeros(BLOCK)
    sentinel = np.full(BLOCK * 2, 0x5A, dtype=np.uint8)
    calls = {
        "gdg_batch_run_shard": lambda: ctx.batch_run_shard(job.inputs, 48000, "lpcm16"),
        "gdg_batch_stream_open_shard": lambda: ctx.batch_stream_open_shard(job.metas, 48000, "lpcm16"),
        "gdg_batch_finish_master:": lambda: ctx.batch_finish_master("lpcm16", [half], [half]),
        "gdg_batch_finish_master_slice": lambda: ctx.batch_finish_master_slice("lpcm16", [half], [half]),
    }
    for name, call in calls.items():
        with pytest.raises(pkg.GdgError, match=name + ".*delivery ratio 147/160") as e:
            call()
        assert e.value.code == pkg.GDG_ERR_UNSUPPORTED, name
    left, right = sentinel.copy(), sentinel.copy()
    lp, rp = (pkg.C.c_void_p * 1)(half.ctypes.data), (pkg.C.c_void_p * 1)(half.ctypes.data)
    rc = pkg.lib().gdg_batch_finish_master(ctx._h, pkg.WAVE_FORMATS["lpcm16"], lp, rp, 1, None, BLOCK, 48000, 0, left.ctypes.data, right.ctypes.data)
    assert rc == pkg.GDG_ERR_UNSUPPORTED and (left == 0x5A).all() and (right == 0x5A).all()      # nothing is written
    ctx.batch_stream_open(job.metas, 48000, "lpcm16", **KW)
    with pytest.raises(pkg.GdgError, match="set delivery ratio: a streamed batch run is open.*delivery ratio 147/160") as e:
        ctx.batch_set_delivery_ratio(2, 1, 1)
    assert e.value.code == pkg.GDG_ERR_INVALID
    with pytest.raises(pkg.GdgError, match="set delivery: a streamed batch run is open.*delivery ratio 147/160"):
        ctx.batch_set_delivery(1)
    with pytest.raises(pkg.GdgError, match="checkpoint.*delivery ratio 147/160.*version-1") as e:
        ctx.batch_stream_checkpoint()
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    size = pkg.C.c_size_t(0)
    assert pkg.lib().gdg_batch_stream_checkpoint_size(ctx._h, pkg.C.byref(size)) == pkg.GDG_ERR_UNSUPPORTED
    assert "delivery ratio 147/160" in pkg.lib().gdg_last_error(ctx._h).decode()
    ctx.batch_stream_close()
    with pytest.raises(pkg.GdgError, match="resume.*delivery ratio 147/160") as e:
        ctx.batch_stream_resume(job.metas, 48000, "lpcm16", b"\0" * 64, **KW)
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    assert (ctx.batch_delivery(), ctx.batch_delivery_ratio()) == (1, (147, 160))
    outs = ctx.batch_run(job.inputs, 48000, "ieee64", **KW)                  # usable afterwards: the job without its blend
    want = job.delivered(1, 147, 160)
    for r in range(NCH + 3):
        assert np.array_equal(outs[r].view(np.float64), want[r]), r
    ctx.close()
