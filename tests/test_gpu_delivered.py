"""The records of the delivered rows (include/gdg.h, DELIVERED RECORDS) on the device, all 40 bytes of every record against the numpy
restatement (tests/delivered_ref.py) run with the library's own taps: the stand-alone call at every block length at which the kernel takes
another path, on the 16-byte and the 8-byte load path, with non-finite samples; the known answers; a stream continued through the history;
the samples' part against the project's own block statistics; and a batch job whose records are the restatement of the delivered float64
files however the job is cut, with and without outputs; off; what is refused; and a file normalised by the delivered rows' true peak."""
import zlib

import numpy as np
import pytest

import delivered_ref as ref
from helpers import package, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
LENGTHS = [1, 2, 23, 24, 25, 255, 256, 257, 511, 513, 1881, 1882, 2048, 4097, 16384]
SPAN = [0] + list(np.cumsum(LENGTHS))


@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def taps():
    return package().true_peak_taps()


@pytest.fixture(scope="module")
def noise():
    """3 rows of noise that clips now and then, one row with a NaN and an inf; the restatement's records of the one call"""
    rng = np.random.default_rng(0xde11)
    x = rng.uniform(-1.05, 1.05, (3, SPAN[-1]))
    x[1, 300] = np.nan
    x[1, 5000] = np.inf
    x[1, SPAN[10] - 1] = -np.inf                                             # the last sample in front of a block: its lead-in
    return x, ref.block_delivered(x, SPAN, package().true_peak_taps())


def same(got, want):
    return got.shape == want.shape and got.tobytes() == want.tobytes()


def on_device(ctx, x, span, stride, skew, hist=None):
    """the device form on rows `stride` apart, the first `skew` doubles behind a 16-byte boundary, NaN around every row"""
    n, samples = x.shape
    nb = len(span) - 1
    d_in, d_rec, d_hist = ctx.alloc(1, n * stride + 2), ctx.alloc(n, nb * 5), ctx.alloc(n, ref.HISTORY)
    padded = np.full(n * stride + 2, np.nan)
    for r in range(n):
        padded[skew + r * stride:skew + r * stride + samples] = x[r]
    d_in.upload(padded.reshape(1, -1))
    d_rec.upload(np.full((n, nb * 5), np.nan))
    if hist is not None:
        d_hist.upload(hist)
    ctx.block_delivered_rows_device(d_in.ptr + 8 * skew, stride, n, samples, span, d_hist.ptr if hist is not None else None, d_rec.ptr)
    got, after = d_rec.download().view(ref.DTYPE).reshape(n, nb), d_hist.download()
    for b in (d_in, d_rec, d_hist):
        b.free()
    return got, after


# ---- 1: the stand-alone call ---------------------------------------------------------------------------------------------------------------
def test_every_block_length_on_both_load_paths(ctx1, noise):
    x, want = noise
    assert SPAN[-1] % 2 == 1                                                 # the host form's rows are an odd stride apart: 8-byte loads
    got = ctx1.block_delivered_rows(x, SPAN)
    assert got.dtype == package().BLOCK_DELIVERED_DTYPE == ref.DTYPE
    for r in range(3):
        for k in range(len(LENGTHS)):
            assert got[r, k].tobytes() == want[r, k].tobytes(), (r, LENGTHS[k], got[r, k], want[r, k])
    assert want["clipped"].sum() > 0 and want["overs"].sum() > 0 and (want["position"] < 0).any()
    # an even stride from a 16-byte boundary: blocks that begin at an even sample take 16-byte loads, the others 8-byte loads; then 8 bytes off
    for stride, skew in ((SPAN[-1] + 9, 0), (SPAN[-1] + 9, 1), (SPAN[-1] + 8, 0)):
        got, _ = on_device(ctx1, x, SPAN, stride, skew)
        assert same(got, want), (stride, skew)
    hist = np.random.default_rng(5).uniform(-1.0, 1.0, (3, ref.HISTORY))
    hist[2, 20] = np.nan
    want_h = hist.copy()
    want_rec = ref.block_delivered(x, SPAN, package().true_peak_taps(), want_h)
    got, after = on_device(ctx1, x, SPAN, SPAN[-1] + 9, 0, hist)
    assert same(got, want_rec) and after.tobytes() == want_h.tobytes()
    assert not same(want_rec[:, :3], want[:, :3])                            # the history is read


def test_known_answers(ctx1, taps):
    silent = ctx1.block_delivered_rows(np.zeros(3000), [0, 1000, 3000])
    assert silent.tobytes() == bytes(silent.nbytes)
    x = np.zeros(3 * 1882)
    o = 1882
    x[o + 100] = 1.0
    rec = ctx1.block_delivered_rows(x, [0, o, 2 * o, 3 * o])[0]
    assert (rec[1]["true_peak"], rec[1]["position"], rec[1]["overs"], rec[1]["peak_index"]) == (1.0, 400, 0, 100)
    assert rec[0]["true_peak"] == 0.0 and rec[2]["true_peak"] == 0.0
    x = np.zeros(3 * 1882)
    x[o - 1] = x[o] = 0.8
    rec = ctx1.block_delivered_rows(x, [0, o, 2 * o, 3 * o])[0]
    centre = 0.8 * taps[1, 11] + 0.8 * taps[1, 12]
    assert abs(taps[1, 11] - 0.633825) < 1e-6 and taps[1, 11] == taps[1, 12] and abs(centre - 1.0141) < 1e-4
    assert rec[1]["peak"] == 0.8 and rec[1]["true_peak"] > 1.0 and abs(rec[1]["true_peak"] - centre) <= 2 ** -51
    assert (rec[1]["position"], rec[1]["overs"], rec[1]["peak_index"]) == (-2, 1, 0)
    assert (rec[0]["true_peak"], rec[0]["peak"], rec[0]["overs"]) == (0.8, 0.8, 0)
    assert same(rec[None, :], ref.block_delivered(x, [0, o, 2 * o, 3 * o], taps))
    # the hole: the stateless record sees neither block's boundary interval
    for part in (x[:o], x[o:2 * o]):
        alone = ctx1.block_true_peak(part)[0, 0]
        assert alone["true_peak"] == 0.8 and alone["overs"] == 0


def test_two_calls_through_the_history_are_the_one_call(ctx1, noise):
    x, want = noise
    for cut in (10, SPAN[11]):                                               # a first call shorter than the history; a block boundary
        hist = np.zeros((3, ref.HISTORY))
        if cut == 10:
            first = ctx1.block_delivered_rows(x[:, :cut], [0, 1, 3, 10], hist)
            span2 = [0] + [s - cut for s in SPAN if s > cut]
            rest = ctx1.block_delivered_rows(x[:, cut:], span2, hist)
            assert same(first[:, :2], want[:, :2]) and same(rest[:, 1:], want[:, 3:])
        else:
            k = SPAN.index(cut)
            first = ctx1.block_delivered_rows(x[:, :cut], SPAN[:k + 1], hist)
            rest = ctx1.block_delivered_rows(x[:, cut:], [s - cut for s in SPAN[k:]], hist)
            assert same(np.concatenate([first, rest], axis=1), want), cut
        assert np.array_equal(hist, x[:, -ref.HISTORY:], equal_nan=True)


def test_the_samples_part_is_the_block_statistics(ctx1, noise):
    x = noise[0][:, :5 * 2048]
    got = ctx1.block_delivered_rows(x, list(range(0, 5 * 2048 + 1, 2048)))
    stats = ctx1.block_stats(x, 2048)
    for name in ("peak", "peak_index", "sum_sq", "clipped"):
        assert np.array_equal(got[name], stats[name]), name


def test_standalone_refusals(ctx1):
    pkg = package()
    x = np.zeros(20000)
    for span, text in (([0, 10, 10, 20000], "block 1"), ([0, 20000], "block 0"), ([1, 20000], "spans run from 1"), ([0, 100], "spans run from 0 to 100"), ([0, 300, 200, 20000], "block 1")):
        with pytest.raises(pkg.GdgError, match="block out rows.*" + text) as e:
            ctx1.block_delivered_rows(x, span)
        assert e.value.code == pkg.GDG_ERR_INVALID
    assert ctx1.block_delivered_rows(x, [0, 16384, 20000]).shape == (1, 2)


# ---- 2: the batch job ----------------------------------------------------------------------------------------------------------------------
NCH, BLOCKS, RATE = 3, 5, 96000
KW = dict(metronome_to_master=True)
BLENDS = [[(0, 0.6), (1, -0.4)]]
NP = NCH + 3 + len(BLENDS)
TRIM = np.array([0.5, -1.0, 0.25, 0.9, -0.7, 1.5])
DELIVERIES = [None, (2, 1, 1), (4, 1, 1), (4, 147, 160), (2, 160, 147)]


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """3 channels, 4 * 8192 + 1000 samples: 5 blocks; metronome to master; one two-term blend"""

    def __init__(self):
        self.pkg = package()
        samples = (BLOCKS - 1) * BLOCK + 1000
        self.inputs = [(lpcm16_file(0.5 * synth_signal(c, samples, RATE)), "lpcm16", RATE) for c in range(NCH)]
        self.metas = [(samples, "lpcm16", RATE)] * NCH
        self.cache = {}

    def configured(self, window=4, delivery=None, gains=False, records=True):
        ctx = self.pkg.Context(NCH, BLOCK)
        ctx.append_unit(0, "overdrive", params=[0, 20, 100, 0, 1, 2])
        ctx.append_unit(1, "tone_stack")
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(NCH):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * c, 1.0 + 0.5 * c, 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
        ctx.metronome_configure(4, 150, RATE)
        ctx.set_window(window)
        ctx.batch_set_blends(BLENDS, [0.8] if gains else None)
        if gains:
            ctx.batch_set_trim(TRIM[:NCH], *TRIM[NCH:])
        if delivery is not None:
            ctx.batch_set_delivery_ratio(*delivery)
        if records:
            ctx.batch_delivered_enable()
        return ctx

    def reference(self, delivery):
        """gains of 1, IEEE64: the files ARE the delivered rows; the library's records of that run and the restatement's of the files"""
        if delivery not in self.cache:
            ctx = self.configured(delivery=delivery)
            outs = ctx.batch_run(self.inputs, RATE, "ieee64", **KW)
            got = ctx.batch_delivered()
            ctx.close()
            rows = np.stack([o.view(np.float64) for o in outs])
            span = ref.spans(*(delivery or (1, 1, 1)), 0, BLOCKS, self.pkg.batch_delivery_samples)
            assert rows.shape == (NP, span[-1]) and all(r.any() for r in rows)
            self.cache[delivery] = (got, ref.block_delivered(rows, span, self.pkg.true_peak_taps()), outs)
        return self.cache[delivery]


@pytest.fixture(scope="module")
def job():
    return Job()


@pytest.mark.parametrize("delivery", DELIVERIES)
def test_the_records_are_the_restatement_of_the_files(job, delivery):
    got, want, _ = job.reference(delivery)
    assert got.shape == (NP, BLOCKS)
    for r in range(NP):
        for k in range(BLOCKS):
            assert got[r, k].tobytes() == want[r, k].tobytes(), (delivery, r, k, got[r, k], want[r, k])
    assert (got["true_peak"] >= got["peak"]).all() and got["peak"].max(axis=1).min() > 0.0      # no port is silent throughout


@pytest.mark.parametrize("delivery", DELIVERIES)
def test_every_cut_keeps_the_same_records(job, delivery):
    want = job.reference(delivery)[0].tobytes()
    for window in (2, 16):
        ctx = job.configured(window=window, delivery=delivery)
        ctx.batch_run(job.inputs, RATE, "ieee64", **KW)
        assert ctx.batch_delivered().tobytes() == want, (delivery, window)
        ctx.close()
    ctx = job.configured(delivery=delivery)
    left = [2, 3]
    pieces = []
    for _ in ctx.batch_stream(job.inputs, RATE, "ieee64", lambda _left: left.pop(0), **KW):
        pieces.append(ctx.batch_delivered())
    assert [p.shape for p in pieces] == [(NP, 2), (NP, 3)] and np.concatenate(pieces, axis=1).tobytes() == want, delivery
    ctx.close()
    ctx = job.configured(delivery=delivery)
    assert ctx.batch_run(job.inputs, RATE, "ieee64", skip_outputs=True, **KW) is None      # the measuring pass: the delivery stages run all the same
    assert ctx.batch_delivered().tobytes() == want, delivery
    ctx.close()
    # a trim and a blend gain: the records are taken in front of them
    ctx = job.configured(delivery=delivery, gains=True)
    outs = ctx.batch_run(job.inputs, RATE, "ieee64", **KW)
    assert ctx.batch_delivered().tobytes() == want, delivery
    ctx.close()
    plain = job.reference(delivery)[2]
    assert np.array_equal(outs[1].view(np.float64), -plain[1].view(np.float64)) and not np.array_equal(outs[0], plain[0])


def crc(outs):
    c = 0
    for o in outs:
        c = zlib.crc32(o.tobytes(), c)
    return c


def test_off_is_off(job):
    """never set, and set and cleared again: the memory and the files of a context that never heard of the switch (a context's second job
    continues its units' state, so the second jobs are compared)"""
    never = job.configured(delivery=(4, 147, 160), gains=True, records=False)
    a1 = never.batch_run(job.inputs, RATE, "lpcm24", **KW)
    a2 = never.batch_run(job.inputs, RATE, "lpcm24", **KW)
    kib = never.get_option("stat_batch_device_kib")
    with pytest.raises(job.pkg.GdgError, match="no records of the delivered rows.*gdg_batch_out_records_enable comes before the call"):
        never.batch_delivered()
    never.close()
    ctx = job.configured(delivery=(4, 147, 160), gains=True, records=True)
    on = ctx.batch_run(job.inputs, RATE, "lpcm24", **KW)
    assert ctx.get_option("stat_batch_device_kib") > kib and crc(on) == crc(a1)     # on: more memory, the same files
    ctx.batch_delivered_enable(False)
    b = ctx.batch_run(job.inputs, RATE, "lpcm24", **KW)
    assert ctx.get_option("stat_batch_device_kib") == kib > 0 and crc(b) == crc(a2) != crc(a1)
    with pytest.raises(job.pkg.GdgError, match="no records of the delivered rows"):
        ctx.batch_delivered()
    ctx.close()


def test_refusals_name_the_switch(job):
    pkg = job.pkg
    ctx = job.configured()
    ctx.batch_set_blends(None)
    half = np.zeros(BLOCK)
    calls = {
        "gdg_batch_run_shard": lambda: ctx.batch_run_shard(job.inputs, RATE, "lpcm16"),
        "gdg_batch_stream_open_shard": lambda: ctx.batch_stream_open_shard(job.metas, RATE, "lpcm16"),
        "gdg_batch_finish_master:": lambda: ctx.batch_finish_master("lpcm16", [half], [half]),
        "gdg_batch_finish_master_slice": lambda: ctx.batch_finish_master_slice("lpcm16", [half], [half]),
    }
    for name, call in calls.items():
        with pytest.raises(pkg.GdgError, match=name + ".*gdg_batch_out_records_enable") as e:
            call()
        assert e.value.code == pkg.GDG_ERR_UNSUPPORTED, name
    ctx.batch_stream_open(job.metas, RATE, "lpcm16", **KW)
    with pytest.raises(pkg.GdgError, match="batch out records: a streamed batch run is open") as e:
        ctx.batch_delivered_enable(False)
    assert e.value.code == pkg.GDG_ERR_INVALID
    with pytest.raises(pkg.GdgError, match="checkpoint.*gdg_batch_out_records_enable.*version-1") as e:
        ctx.batch_stream_checkpoint()
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    ctx.batch_stream_close()
    with pytest.raises(pkg.GdgError, match="resume.*gdg_batch_out_records_enable") as e:
        ctx.batch_stream_resume(job.metas, RATE, "lpcm16", b"\0" * 64, **KW)
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    ctx.batch_run(job.inputs, RATE, "ieee64", **KW)                          # usable afterwards
    assert ctx.batch_delivered().shape == (NCH + 3, BLOCKS)
    ctx.close()


# ---- 3: a file normalised by what is written -----------------------------------------------------------------------------------------------
def test_render_normalized_by_the_delivered_rows_meets_the_target(ctx1):
    """a full-scale square-like burst overshoots behind the band-limiting filters; with measure="delivered" the file's own records, measured
    again, lie at or below the target times (1 + 2^-50); the default measure="render" plans and writes what it did before"""
    import __graft_entry__ as entry
    pkg = entry.load_package()                                              # build() has made both libraries
    from go_dsp_guitar_amd import host
    nch, rate, blocks, delivery = 2, 192000, 3, (4, 147, 160)
    n = np.arange(blocks * BLOCK - 500)
    burst = 0.98 * np.sign(np.sin(2 * np.pi * 3000.0 * n / rate)) * ((n > 3000) & (n < 2 * BLOCK + 100))
    inputs = [(lpcm16_file(burst), "lpcm16", rate), (lpcm16_file(0.3 * synth_signal(1, n.size, rate)), "lpcm16", rate)]

    def engine():
        eng = host.Engine(nch, BLOCK)
        chains = [eng.create_chain(host.ImpulseResponses()) for _ in range(nch)]
        sp = host.Spatializer(eng, nch)
        sp.SetSampleRate(rate)
        for c in range(nch):
            sp.SetAzimuth(c, -30.0 + 60.0 * c); sp.SetDistance(c, 1.0); sp.SetLevel(c, 0.9)
        return eng, (chains, sp)

    target = 10.0 ** (-1.0 / 20.0)
    span = ref.spans(*delivery, 0, blocks, pkg.batch_delivery_samples)
    eng, keep = engine()
    outs, gains = eng.render_normalized(-1.0, 40.0, inputs, rate, "ieee64", window=2, deliver=delivery, measure="delivered")
    assert eng.last_error() == ""
    rec = eng.normalize_delivered
    assert rec.shape == (nch + 3, blocks) and rec.dtype == pkg.BLOCK_DELIVERED_DTYPE
    assert gains.tobytes() == pkg.trim_from_delivered(rec, target, 100.0).tobytes()
    rows = np.stack([o.view(np.float64) for o in outs])
    assert rows.shape == (nch + 3, span[-1])
    again = ctx1.block_delivered_rows(rows, span)
    worst = again["true_peak"].max(axis=1)
    print("delivered true peaks over the target:", worst / target - 1.0, "gains", gains)
    assert rec["true_peak"][0].max() > 0.98                                 # the burst overshoots behind the filters
    for r in range(nch + 3):
        assert worst[r] <= target * (1.0 + 2.0 ** -50), (r, worst[r] / target - 1.0)
        if 1.0 < gains[r] < 100.0 or 0.0 < gains[r] < 1.0:
            assert worst[r] >= target * (1.0 - 2.0 ** -40), r               # ... and reach it: the gain was planned from these rows
    del keep
    # the default: gains from the session-rate records, the bytes of a plain two-pass run
    eng, keep = engine()
    outs_r, gains_r = eng.render_normalized(-1.0, 40.0, inputs, rate, "ieee64", window=2, deliver=delivery)
    assert eng.normalize_delivered is None and gains_r.tobytes() == pkg.trim_from_true_peak(eng.normalize_true_peak, target, 100.0).tobytes()
    assert not np.array_equal(gains_r, gains)
    del keep
    eng, keep = engine()
    plain = eng.batch_run(inputs, rate, "ieee64", window=2, deliver=delivery, trim=gains_r)
    for r in range(nch + 3):
        assert np.array_equal(plain[r], outs_r[r]), r
    del keep
