"""The delivery at a half or a quarter of the session rate (include/gdg.h, DELIVERY) on the device, bit for bit against the numpy restatement
of the stated arithmetic (tests/deliver_ref.py): the stand-alone kernel at every size at which it takes another path, with and without a
history, continued through it, with sentinels around what it may write; a batch job of 3 channels and 4 blocks whose every port -- chain
outputs, master left and right, metronome, a two-term blend -- equals the restatement of its session-rate row however the job is cut; the
encoders behind it (plain, and dither + trim + blend gain with the index counted in delivered samples); the records, which stay those of
the render; off; and what is refused."""
import numpy as np
import pytest

import deliver_ref as ref
import dither_ref
from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
RATE, NCH, BLOCKS, SEED = 48000, 3, 4, 0x51c7e9a30b2d4f68
SAMPLES = 3 * BLOCK + 1000
LEVEL = 0.1
KW = dict(metronome_to_master=True)
BLENDS = [[(0, 0.6), (1, -0.4)]]
BLEND_GAIN = [0.8]
TRIM = np.array([0.5, -1.0, 1.7, 0.9, -0.7, 1.5])
NP = NCH + 3 + len(BLENDS)
PORTS = list(range(NCH)) + [dither_ref.PORT_LEFT, dither_ref.PORT_RIGHT, dither_ref.PORT_METRONOME, NCH + 3]


@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


# ---- 1: the stand-alone kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [2, 4])
def test_known_answers(ctx1, factor):
    h = ref.taps(factor)
    assert np.array_equal(package().deliver_taps(factor), h)
    n = factor * 64
    for at in (0, 1):
        x = np.zeros(n)
        x[at] = 1.0
        want = np.array([ref.A * h[factor * i - at] if 0 <= factor * i - at < h.size else 0.0 for i in range(n // factor)])
        got = ctx1.deliver_rows(x, factor)
        assert np.array_equal(got, want), (factor, at)
    y = ctx1.deliver_rows(np.zeros(n), factor)
    assert not y.any() and not np.signbit(y).any()                          # silence: exactly +0.0


@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("n_rows", [1, 3])
def test_rows_against_the_restatement_with_sentinels(ctx1, factor, n_rows):
    rng = np.random.default_rng(100 * factor + n_rows)
    for samples in (factor, 3 * factor, BLOCK, BLOCK + factor):
        stride, out_stride = (samples + 7 if n_rows > 1 else samples), samples // factor + 5
        x = rng.uniform(-1.0, 1.0, (n_rows, samples))
        for with_history in (False, True):
            hist = rng.uniform(-1.0, 1.0, (n_rows, ref.HISTORY)) if with_history else None
            d_in, d_out, d_hist = ctx1.alloc(n_rows, stride), ctx1.alloc(n_rows, out_stride), ctx1.alloc(n_rows, ref.HISTORY)
            padded = np.full((n_rows, stride), np.nan)
            padded[:, :samples] = x
            d_in.upload(padded)
            d_out.upload(np.full((n_rows, out_stride), np.nan))
            if with_history:
                d_hist.upload(hist)
            ctx1.deliver_rows_device(d_in.ptr, stride, n_rows, samples, factor, d_hist.ptr if with_history else None, d_out.ptr, out_stride)
            got, after = d_out.download(), d_hist.download()
            for b in (d_in, d_out, d_hist):
                b.free()
            want = ref.deliver(x, factor, hist)
            assert np.array_equal(got[:, :samples // factor], want), (factor, n_rows, samples, with_history)
            assert np.isnan(got[:, samples // factor:]).all(), "samples behind the delivered row were written"
            if with_history:                                                # the last 154 of [history | x]: shifted old ones when samples < 154
                assert np.array_equal(after, ref.next_history(x, hist)), (factor, n_rows, samples)
            # the host form, compact rows
            h2 = None if hist is None else hist.copy()
            assert np.array_equal(ctx1.deliver_rows(x, factor, h2), want)
            if with_history:
                assert np.array_equal(h2, ref.next_history(x, hist))


@pytest.mark.parametrize("factor", [2, 4])
def test_two_calls_through_the_history_are_one_call(ctx1, factor):
    x = np.random.default_rng(7 + factor).uniform(-1.0, 1.0, (2, 2 * BLOCK))
    whole = ctx1.deliver_rows(x, factor)
    hist = np.zeros((2, ref.HISTORY))
    parts = [ctx1.deliver_rows(x[:, :BLOCK], factor, hist), ctx1.deliver_rows(x[:, BLOCK:], factor, hist)]
    assert np.array_equal(np.concatenate(parts, axis=1), whole)
    assert np.array_equal(whole, ref.deliver(x, factor))
    assert np.array_equal(ctx1.deliver_rows(x, 1), x)                       # factor 1 copies


def test_standalone_refusals(ctx1):
    pkg = package()
    for factor, samples in ((3, 12), (0, 12), (2, 7), (4, 6)):
        with pytest.raises(pkg.GdgError, match="delivery factor") as e:
            ctx1.deliver_rows(np.zeros(samples), factor)
        assert e.value.code == pkg.GDG_ERR_INVALID
    assert ctx1.deliver_rows(np.zeros(8), 4).size == 2                      # the context is usable afterwards


# ---- 2: the batch job ----------------------------------------------------------------------------------------------------------------------
def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """3 channels at 48 kHz, a short chain each (channel 1 with a 300-tap power amp); 3 * 8192 + 1000 samples: 4 blocks; metronome to master;
    one two-term blend.  Channel 2 reads the file of channel 0, so that the same job can be described with a source map."""

    def __init__(self):
        self.pkg = package()
        files = [lpcm16_file(LEVEL * synth_signal(c, SAMPLES, RATE)) for c in range(2)]
        self.inputs = [(files[0], "lpcm16", RATE), (files[1], "lpcm16", RATE), (files[0], "lpcm16", RATE)]
        self.ir = synth_ir(300, seed=91)
        self.cache = {}

    def configured(self, window=4, factor=None, shaped=False, records=False, sources=False):
        ctx = self.pkg.Context(NCH, BLOCK)
        ctx.append_unit(0, "overdrive", params=[0, 20, 100, 0, 1, 2])
        ctx.append_unit(1, "power_amp", fir=self.ir)
        ctx.append_unit(2, "tone_stack")
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(NCH):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * c, 1.0 + 0.5 * c, 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
        ctx.metronome_configure(4, 150, RATE)
        ctx.set_window(window)
        ctx.batch_set_blends(BLENDS, BLEND_GAIN if shaped else None)
        if shaped:
            ctx.batch_set_dither(1, SEED, 0)
            ctx.batch_set_trim(TRIM[:NCH], *TRIM[NCH:])
        if records:
            ctx.batch_report_enable()
            ctx.batch_spectrum_enable([100.0, 400.0, 1600.0, 6400.0])
            ctx.batch_true_peak_enable()
        if sources:
            ctx.batch_set_sources([0, 1, 0])
        if factor is not None:
            ctx.batch_set_delivery(factor)
        return ctx

    def run(self, fmt, factor=None, shaped=False, records=False):
        key = (fmt, factor, shaped, records)
        if key not in self.cache:
            ctx = self.configured(factor=factor, shaped=shaped, records=records)
            outs = ctx.batch_run(self.inputs, RATE, fmt, **KW)
            res = dict(outs=outs, kib=ctx.get_option("stat_batch_device_kib"))
            if records:
                res.update(report=ctx.batch_report().tobytes(), spectrum=ctx.batch_spectrum().tobytes(), true_peak=ctx.batch_true_peak().tobytes())
            ctx.close()
            self.cache[key] = res
        return self.cache[key]

    def rows(self):
        """the float64 rows of the job at the session rate: an IEEE64 render without delivery (whose bytes ARE the rows)"""
        rows = [o.view(np.float64) for o in self.run("ieee64")["outs"]]
        assert len(rows) == NP and all(r.size == BLOCKS * BLOCK and r.any() for r in rows)
        return rows

    def delivered(self, factor):
        return [ref.deliver(r, factor) for r in self.rows()]


@pytest.fixture(scope="module")
def job():
    return Job()


@pytest.mark.parametrize("factor", [2, 4])
def test_every_port_is_the_restatement_of_its_row(job, factor):
    outs = job.run("ieee64", factor)["outs"]
    want = job.delivered(factor)
    assert len(outs) == NP
    for r in range(NP):
        got = outs[r].view(np.float64)
        assert got.size == BLOCKS * BLOCK // factor
        assert np.array_equal(got, want[r]), "factor %d, port %d: %d samples differ" % (factor, r, np.count_nonzero(got != want[r]))


@pytest.mark.parametrize("factor", [2, 4])
def test_the_encoders_read_the_delivered_rows(job, factor):
    enc = job.configured(window=1)
    want = job.delivered(factor)
    plain = job.run("lpcm24", factor)["outs"]
    shaped = job.run("lpcm24", factor, shaped=True)["outs"]
    gains = list(TRIM) + BLEND_GAIN
    for r in range(NP):
        assert np.array_equal(plain[r], enc.wave_encode("lpcm24", want[r])), (factor, r)
        # dither, trim and blend gain on: sample i of the delivered row has the index i of the delivered job
        assert np.array_equal(shaped[r], enc.wave_encode_trim("lpcm24", want[r], gains[r], 1, SEED, PORTS[r], 0)), (factor, r)
    assert not np.array_equal(plain[0], shaped[0])
    enc.close()


@pytest.mark.parametrize("factor", [2, 4])
def test_every_cut_writes_the_same_bytes(job, factor):
    want = job.run("lpcm24", factor, shaped=True)["outs"]
    sizes = []
    for window, sources, slices in ((1, False, None), (4, True, None), (4, False, [1, 1, 1, 1]), (1, True, [2, 1, 1]), (4, False, [2, 1, 1])):
        ctx = job.configured(window=window, factor=factor, shaped=True, sources=sources)
        inputs = [job.inputs[0], job.inputs[1], None] if sources else job.inputs
        if slices is None:
            got = ctx.batch_run(inputs, RATE, "lpcm24", **KW)
        else:
            left = list(slices)
            pieces = list(ctx.batch_stream(inputs, RATE, "lpcm24", lambda _left: left.pop(0), **KW))
            assert [p[0].size for p in pieces] == [b * BLOCK // factor * 3 for b in slices]
            got = [np.concatenate([p[r] for p in pieces]) for r in range(NP)]
        sizes.append(ctx.get_option("stat_batch_device_kib"))
        ctx.close()
        for r in range(NP):
            assert np.array_equal(got[r], want[r]), (factor, window, sources, slices, r)


def test_the_records_are_those_of_the_render(job):
    never = job.run("lpcm16", records=True)
    for factor in (2, 4):
        with_it = job.run("lpcm16", factor, records=True)
        for kind in ("report", "spectrum", "true_peak"):
            assert with_it[kind] == never[kind], (factor, kind)
        assert with_it["outs"][0].size == never["outs"][0].size // factor


def test_factor_one_is_off_and_the_buffers_go(job):
    never = job.run("lpcm24", shaped=True)
    one = job.run("lpcm24", 1, shaped=True)
    for r in range(NP):
        assert np.array_equal(one["outs"][r], never["outs"][r]), r
    assert one["kib"] == never["kib"] and never["kib"] > 0
    ctx = job.configured(factor=4, shaped=True)
    assert ctx.batch_delivery() == 4
    at4 = ctx.batch_run(job.inputs, RATE, "lpcm24", **KW)
    assert at4[0].size * 4 == never["outs"][0].size
    ctx.batch_set_delivery(1)
    assert ctx.batch_delivery() == 1
    back = ctx.batch_run(job.inputs, RATE, "lpcm24", **KW)
    # the units, the spatializer and the metronome go on from the first job: the second job of a context that never heard of the call
    plain = job.configured(shaped=True)
    plain.batch_run(job.inputs, RATE, "lpcm24", **KW)
    second = plain.batch_run(job.inputs, RATE, "lpcm24", **KW)
    for r in range(NP):
        assert np.array_equal(back[r], second[r]), r
    assert ctx.get_option("stat_batch_device_kib") == plain.get_option("stat_batch_device_kib") == never["kib"]      # the scratch rows and the history are released
    ctx.close()
    plain.close()


def test_refusals_name_the_factor_and_leave_the_context_usable(job):
    pkg = job.pkg
    ctx = job.configured(factor=2)
    ctx.batch_set_blends(None)
    for bad in (0, 3):
        with pytest.raises(pkg.GdgError, match="delivery factor %d" % bad) as e:
            ctx.batch_set_delivery(bad)
        assert e.value.code == pkg.GDG_ERR_INVALID and ctx.batch_delivery() == 2
    half = np.zeros(BLOCK)
    calls = {
        "gdg_batch_run_shard": lambda: ctx.batch_run_shard(job.inputs, RATE, "lpcm16"),
        "gdg_batch_stream_open_shard": lambda: ctx.batch_stream_open_shard([(SAMPLES, "lpcm16", RATE)] * NCH, RATE, "lpcm16"),
        "gdg_batch_finish_master:": lambda: ctx.batch_finish_master("lpcm16", [half], [half]),
        "gdg_batch_finish_master_slice": lambda: ctx.batch_finish_master_slice("lpcm16", [half], [half]),
    }
    for name, call in calls.items():
        with pytest.raises(pkg.GdgError, match=name + ".*delivery factor 2") as e:
            call()
        assert e.value.code == pkg.GDG_ERR_UNSUPPORTED, name
    ctx.batch_stream_open([(SAMPLES, "lpcm16", RATE)] * NCH, RATE, "lpcm16", **KW)
    with pytest.raises(pkg.GdgError, match="set delivery: a streamed batch run is open.*delivery factor 2") as e:
        ctx.batch_set_delivery(4)
    assert e.value.code == pkg.GDG_ERR_INVALID
    with pytest.raises(pkg.GdgError, match="checkpoint.*delivery factor 2.*version-1") as e:
        ctx.batch_stream_checkpoint()
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    size = pkg.C.c_size_t(0)
    assert pkg.lib().gdg_batch_stream_checkpoint_size(ctx._h, pkg.C.byref(size)) == pkg.GDG_ERR_UNSUPPORTED
    assert "delivery factor 2" in pkg.lib().gdg_last_error(ctx._h).decode()
    ctx.batch_stream_close()
    outs = ctx.batch_run(job.inputs, RATE, "ieee64", **KW)                   # usable afterwards: the job without its blend
    want = job.delivered(2)
    for r in range(NCH + 3):
        assert np.array_equal(outs[r].view(np.float64), want[r]), r
    ctx.close()
