"""The output trim (gdg_batch_set_trim, gdg_wave_encode_trim) on the device, byte for byte against the numpy restatement of the arithmetic
include/gdg.h states (tests/trim_ref.py): every encoding place of the batch engine -- one-call run, windows, slices, a resumed checkpoint,
a source map, shards with their metronome and both forms of the master finish -- in all six formats with dither off and on; that gain 1.0
is off; that every record, the meters, a shard's float64 partials and the state are those of the render; what is refused; and the two-pass
helper of the C++ twin.  The float64 rows the encoder sees come from a run of the same job on a fresh context with IEEE64 out and no trim
(whose bytes ARE the rows)."""
import numpy as np
import pytest

import dither_ref
import trim_ref as ref
from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
RATE, NCH, SEED = 48000, 3, 0x7219a5c3e1d0f864
SAMPLES, BLOCKS = 2 * BLOCK + 100, 3
KW = dict(metronome_to_master=True)
PORTS = list(range(NCH)) + [dither_ref.PORT_LEFT, dither_ref.PORT_RIGHT, dither_ref.PORT_METRONOME]
# chain 0, 1, 2, master left, master right, metronome: the metronome's ramps peak at 0.5, so its 3.0 drives the clamp
GAINS = np.array([0.5, -1.0, 1.7, 0.0, -1.7, 3.0])
LEVEL = 0.1                                                                 # of the inputs: no output row of the job passes full scale


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """3 channels, each a 300-tap power amp; 2 * 8192 + 100 samples: 3 blocks; window 2; metronome to master.  Channel 2 reads the file
    of channel 0 through another amp, so that the same job can be described with a source map."""

    def __init__(self):
        self.pkg = package()
        files = [lpcm16_file(LEVEL * synth_signal(c, SAMPLES, RATE)) for c in range(2)]
        self.inputs = [(files[0], "lpcm16", RATE), (files[1], "lpcm16", RATE), (files[0], "lpcm16", RATE)]
        self.irs = [synth_ir(300, seed=80 + c) for c in range(NCH)]
        self.cache = {}

    def configured(self, first=0, count=NCH, window=2):
        ctx = self.pkg.Context(count, BLOCK)
        for c in range(count):
            ctx.append_unit(c, "power_amp", fir=self.irs[first + c])
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(count):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * (first + c), 1.0 + 0.5 * (first + c), 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
        ctx.metronome_configure(4, 150, RATE)
        ctx.set_window(window)
        return ctx

    def setup(self, ctx, dither, gains, first=0, count=NCH, wide=True):
        """dither: None or the seed; gains: None (never set) or the job's six -- the context gets its channels' and, when `wide`, the job-wide ones"""
        if dither is not None:
            ctx.batch_set_dither(1, dither, first)
        if gains is not None:
            g = np.asarray(gains, dtype=np.float64)
            ctx.batch_set_trim(g[first:first + count], *(g[NCH:] if wide else (1.0, 1.0, 1.0)))

    def run(self, fmt, dither=None, gains=None, records=False):
        """the one-call run on a fresh context -> dict(outs, kib and, with records, everything a batch call can be asked to keep)"""
        key = (fmt, dither, None if gains is None else tuple(gains), records)
        if key not in self.cache:
            ctx = self.configured()
            self.setup(ctx, dither, gains)
            if records:
                ctx.batch_report_enable()
                ctx.batch_spectrum_enable([100.0, 400.0, 1600.0, 6400.0])
                ctx.batch_align_enable([-1, 0, 0, -1, NCH, -1], 64)
                ctx.batch_true_peak_enable()
                ctx.meter_configure(2 * NCH + 3)
                ctx.meter_set_enabled(True)
            outs = ctx.batch_run(self.inputs, RATE, fmt, run_meters=records, **KW)
            res = dict(outs=outs, kib=ctx.get_option("stat_batch_device_kib"))
            if records:
                res.update(report=ctx.batch_report(), spectrum=ctx.batch_spectrum().tobytes(), align=ctx.batch_align().tobytes(),
                           true_peak=ctx.batch_true_peak().tobytes(), meters=[ctx.meter_state(p) for p in range(2 * NCH + 3)], state=bytes(ctx.save_state()))
            ctx.close()
            self.cache[key] = res
        return self.cache[key]

    def rows(self):
        """the float64 rows of the job, from an IEEE64 render without a trim; first of all they do not clip (a condition on the inputs)"""
        ref_run = self.run("ieee64", records=True)
        report = ref_run["report"]
        assert report.shape == (NCH + 3, BLOCKS) and not report["clipped"].any() and not report["nonfinite"].any(), report["clipped"]
        rows = [o.view(np.float64) for o in ref_run["outs"]]
        assert all(r.size == BLOCKS * BLOCK and r.any() for r in rows)
        return rows


@pytest.fixture(scope="module")
def job():
    return Job()


def want_files(job, fmt, dither, gains=GAINS):
    return [ref.encode(fmt, row, gains[r], dither, PORTS[r], 0) for r, row in enumerate(job.rows())]


# ---- 1: exactness ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_trimmed_files_are_the_restatement_of_the_rows(job, fmt):
    rows = job.rows()
    assert 3.0 * np.abs(rows[NCH + 2]).max() > 1.0 and 1.7 * np.abs(rows[2]).max() < 1.0          # the 3.0 drives the clamp, the 1.7 does not
    for dither in (None, SEED):
        outs = job.run(fmt, dither, GAINS)["outs"]
        want = want_files(job, fmt, dither)
        for r in range(NCH + 3):
            assert outs[r].size == want[r].size and np.array_equal(outs[r], want[r]), "%s, dither %s, output %d (gain %g): %d bytes differ" % (
                fmt, dither is not None, r, GAINS[r], np.count_nonzero(outs[r] != want[r]))
    if fmt in dither_ref.SCALE:                                             # ... and the trim did something: another file than without it
        assert not np.array_equal(job.run(fmt, None, GAINS)["outs"][0], job.run(fmt)["outs"][0])
        codes = dither_ref.decode_codes(fmt, job.run(fmt, None, GAINS)["outs"][NCH + 2])
        assert codes.max() == dither_ref.RANGE[fmt][1]                       # the metronome's 3.0 reached the top code
        assert not dither_ref.decode_codes(fmt, job.run(fmt, None, GAINS)["outs"][NCH]).any()      # gain 0.0: digital silence


# ---- 2: gain 1.0 is off ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,dither", [("lpcm16", None), ("lpcm24", SEED), ("ieee32", None)])
def test_all_gains_one_is_off(job, fmt, dither):
    never = job.run(fmt, dither)
    ones = job.run(fmt, dither, [1.0] * (NCH + 3))
    for r in range(NCH + 3):
        assert np.array_equal(ones["outs"][r], never["outs"][r]), r
    assert ones["kib"] == never["kib"] and never["kib"] > 0
    assert job.run(fmt, dither, GAINS)["kib"] == never["kib"]               # the gains live outside the batch buffers
    # set and taken back: off again
    ctx = job.configured()
    job.setup(ctx, dither, GAINS)
    ctx.batch_set_trim(None)
    back = ctx.batch_run(job.inputs, RATE, fmt, **KW)
    ctx.close()
    for r in range(NCH + 3):
        assert np.array_equal(back[r], never["outs"][r]), r


# ---- 3: the known answer and the stand-alone form ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


def test_known_answer_and_the_standalone_encoder(ctx1):
    pkg = package()
    # seed 0x63, port 3, index 8192, x = 2e-5, g = 0.5: the header's codes of x = 1e-5
    assert list(dither_ref.decode_codes("lpcm16", ctx1.wave_encode_trim("lpcm16", [2e-5], 0.5, 1, 0x63, 3, 8192))) == [0]
    assert list(dither_ref.decode_codes("lpcm24", ctx1.wave_encode_trim("lpcm24", [2e-5], 0.5, 1, 0x63, 3, 8192))) == [83]
    rng = np.random.default_rng(31)
    x = rng.uniform(-1.2, 1.2, 1027)
    x[::9] = rng.normal(0.0, 1e-4, x[::9].size)
    for fmt in ref.FORMATS:
        for g in (0.5, -1.0, 1.7, 0.0, 3.0):
            for n in (1, 3, 4, 5, 1027):
                for mode in (0, 1):
                    got = ctx1.wave_encode_trim(fmt, x[:n], g, mode, SEED, 7, 2 ** 32 - 3)
                    want = ref.encode(fmt, x[:n], g, SEED if mode else None, 7, 2 ** 32 - 3)
                    assert np.array_equal(got, want), (fmt, g, n, mode)
        # gain 1.0 is gdg_wave_encode_dither's call
        assert np.array_equal(ctx1.wave_encode_trim(fmt, x, 1.0, 1, SEED, 7, 5), ctx1.wave_encode_dither(fmt, x, 1, SEED, 7, 5)), fmt
        assert np.array_equal(ctx1.wave_encode_trim(fmt, x, 1.0, 0, SEED, 7, 5), ctx1.wave_encode(fmt, x)), fmt
    for bad in (float("nan"), float("inf")):
        with pytest.raises(pkg.GdgError, match="not finite") as e:
            ctx1.wave_encode_trim("lpcm16", x, bad)
        assert e.value.code == pkg.GDG_ERR_INVALID


@pytest.mark.parametrize("fmt", ["lpcm8", "lpcm24", "ieee32", "ieee64"])
def test_device_form_takes_both_alignments(ctx1, fmt):
    """input offset by 8 bytes, output by 1: everything goes one sample per thread with byte stores; and the aligned form beside it"""
    pkg = package()
    lib, w = pkg.lib(), ref.WIDTH[fmt]
    x = np.random.default_rng(37).uniform(-1.2, 1.2, 1030)
    for n, mode in ((1, 0), (5, 1), (1027, 0), (1028, 1)):
        d_in, d_out = ctx1.alloc(1, n + 2), ctx1.alloc(1, (n * w + 16 + 7) // 8)
        d_in.upload(np.concatenate([[9.0], x[:n], [9.0]]))
        for in_off, out_off in ((8, 1), (0, 0), (8, 0), (0, 1)):
            d_out.upload(np.zeros(d_out.cols))
            src = np.concatenate([[9.0], x[:n]])[in_off // 8:in_off // 8 + n]
            ctx1.wave_encode_trim_device(fmt, d_in.ptr + in_off, n, d_out.ptr + out_off, -1.7, mode, SEED, 7, 2 ** 40 + 1)
            raw = np.zeros(d_out.cols * 8, dtype=np.uint8)
            ctx1._check(lib.gdg_copy_to_host(ctx1._h, raw.ctypes.data, d_out.ptr, raw.size))
            want = ref.encode(fmt, src, -1.7, SEED if mode else None, 7, 2 ** 40 + 1)
            assert np.array_equal(raw[out_off:out_off + n * w], want), (fmt, n, mode, in_off, out_off)
            assert not raw[:out_off].any() and not raw[out_off + n * w:].any(), "bytes outside the output were written"
        d_in.free()
        d_out.free()


# ---- 4: invariance -----------------------------------------------------------------------------------------------------------------------
FMT = "lpcm24"                                                              # with dither on: both siblings' arguments are in play


def test_window_slices_and_a_resumed_checkpoint_write_the_same_bytes(job):
    pkg = job.pkg
    want = job.run(FMT, SEED, GAINS)["outs"]
    ctx = job.configured(window=1)
    job.setup(ctx, SEED, GAINS)
    got = ctx.batch_run(job.inputs, RATE, FMT, **KW)
    ctx.close()
    for r in range(NCH + 3):
        assert np.array_equal(got[r], want[r]), "window 1, output %d" % r
    ctx = job.configured()
    job.setup(ctx, SEED, GAINS)
    it = iter([1, 2])
    parts = list(ctx.batch_stream(job.inputs, RATE, FMT, lambda left: next(it), **KW))
    ctx.close()
    for r in range(NCH + 3):
        assert np.array_equal(np.concatenate([p[r] for p in parts]), want[r]), "slices of 1 + 2 blocks, output %d" % r
    # slice 1, a checkpoint, and slice 2 on a fresh context on which the trim was set again
    metas = [(SAMPLES, "lpcm16", RATE)] * NCH
    cut = lambda need: [d[0][2 * f:2 * (f + c)] for d, (f, c) in zip(job.inputs, need)]
    ctx = job.configured()
    job.setup(ctx, SEED, GAINS)
    assert ctx.batch_stream_open(metas, RATE, FMT, **KW) == BLOCKS * BLOCK
    head = ctx.batch_stream_step(1, cut(ctx.batch_stream_need(1)))
    blob = ctx.batch_stream_checkpoint()
    ctx.batch_stream_close()
    ctx.close()
    ctx = job.configured()
    job.setup(ctx, SEED, GAINS)
    assert ctx.batch_stream_resume(metas, RATE, FMT, blob, **KW) == BLOCK
    tail = ctx.batch_stream_step(2, cut(ctx.batch_stream_need(2)))
    ctx.batch_stream_close()
    ctx.close()
    for r in range(NCH + 3):
        assert np.array_equal(np.concatenate([head[r], tail[r]]), want[r]), "resumed: output %d" % r
    # ... and without the trim on the target the second slice is another file: the blob does not carry it
    ctx = job.configured()
    job.setup(ctx, SEED, None)
    assert ctx.batch_stream_resume(metas, RATE, FMT, blob, **KW) == BLOCK
    bare = ctx.batch_stream_step(2, cut(ctx.batch_stream_need(2)))
    ctx.batch_stream_close()
    ctx.close()
    assert not np.array_equal(bare[0], tail[0])


def test_a_source_map_writes_the_same_bytes(job):
    want = job.run(FMT, SEED, GAINS)["outs"]
    ctx = job.configured()
    job.setup(ctx, SEED, GAINS)
    ctx.batch_set_sources([0, 1, 0])
    got = ctx.batch_run([job.inputs[0], job.inputs[1], None], RATE, FMT, **KW)
    ctx.close()
    for r in range(NCH + 3):
        assert np.array_equal(got[r], want[r]), r


def test_two_shards_write_the_single_context_files_and_the_finish_trims_its_own_sums(job):
    single = job.run(FMT, SEED, GAINS)["outs"]
    n = BLOCKS * BLOCK
    split = [(0, 2), (2, 1)]
    ctxs = [job.configured(f, c) for f, c in split]
    for g, (ctx, (f, c)) in enumerate(zip(ctxs, split)):
        job.setup(ctx, SEED, GAINS, f, c, wide=(g == 0))                    # shard 0 runs the metronome and finishes the master
    shards = [ctx.batch_run_shard(job.inputs[f:f + c], RATE, FMT, job_samples=n, metronome=(g == 0)) for g, (ctx, (f, c)) in enumerate(zip(ctxs, split))]
    got = shards[0][0] + shards[1][0]
    for c in range(NCH):
        assert np.array_equal(got[c], single[c]), "chain output %d" % c
    assert np.array_equal(shards[0][3], single[NCH + 2]), "the metronome track"
    # the float64 partials and the float64 metronome are those of a shard that never heard of a trim
    bare = job.configured(0, 2)
    plain = bare.batch_run_shard(job.inputs[0:2], RATE, FMT, job_samples=n, metronome=True)
    for k in (1, 2, 4):
        assert np.array_equal(plain[k], shards[0][k]), k
    lefts, rights, aux = [s[1] for s in shards], [s[2] for s in shards], shards[0][4]
    # a sharded sum is associated differently from the single context's: the finish's own sums as IEEE64 (no trim), then their restatement
    sums = [b.view(np.float64) for b in bare.batch_finish_master("ieee64", lefts, rights, aux=aux)]
    bare.close()
    want = [ref.encode(FMT, sums[0], GAINS[NCH], SEED, dither_ref.PORT_LEFT, 0), ref.encode(FMT, sums[1], GAINS[NCH + 1], SEED, dither_ref.PORT_RIGHT, 0)]
    whole = ctxs[0].batch_finish_master(FMT, lefts, rights, aux=aux)
    for side in range(2):
        assert np.array_equal(whole[side], want[side]), "finish_master, side %d" % side
    trimmed64 = [b.view(np.float64) for b in ctxs[0].batch_finish_master("ieee64", lefts, rights, aux=aux)]
    assert np.array_equal(trimmed64[1], sums[1] * GAINS[NCH + 1]) and not trimmed64[0].any()
    ctxs[0].batch_dither_seek(0)
    cut = lambda a, b: dict(lefts=[p[a:b] for p in lefts], rights=[p[a:b] for p in rights], aux=aux[a:b])
    first = ctxs[0].batch_finish_master_slice(FMT, **cut(0, BLOCK))
    second = ctxs[0].batch_finish_master_slice(FMT, **cut(BLOCK, n))
    for side in range(2):
        assert np.array_equal(np.concatenate([first[side], second[side]]), want[side]), "two slices, side %d" % side
    # the plain encoder's finish as well
    ctxs[0].batch_set_dither(0)
    whole = ctxs[0].batch_finish_master("lpcm16", lefts, rights, aux=aux)
    for side in range(2):
        assert np.array_equal(whole[side], ref.encode("lpcm16", sums[side], GAINS[NCH + side])), "plain finish_master, side %d" % side
    for ctx in ctxs:
        ctx.close()


# ---- 5: the records are taken before the trim --------------------------------------------------------------------------------------------
def test_records_meters_partials_and_state_are_those_of_the_render(job):
    off, on = job.run(FMT, SEED, None, records=True), job.run(FMT, SEED, GAINS, records=True)
    assert off["report"].tobytes() == on["report"].tobytes() and len(on["report"].tobytes()) == (NCH + 3) * BLOCKS * 32
    for what in ("spectrum", "align", "true_peak", "meters", "state"):
        assert off[what] == on[what] and len(on[what]) > 0, what
    assert on["kib"] == off["kib"]
    assert not np.array_equal(on["outs"][0], off["outs"][0])


# ---- 6: validation -----------------------------------------------------------------------------------------------------------------------
def test_what_is_refused_leaves_the_setting_in_force(job):
    pkg = job.pkg
    want = job.run("lpcm16", None, GAINS)["outs"]
    ctx = job.configured()
    job.setup(ctx, None, GAINS)
    bad = [(lambda: ctx.batch_set_trim([0.5, float("nan"), 1.0]), r"chain_gain\[1\]"), (lambda: ctx.batch_set_trim([0.5, 1.0, float("inf")]), r"chain_gain\[2\]"),
           (lambda: ctx.batch_set_trim(None, master_right=float("-inf")), "master_right"), (lambda: ctx.batch_set_trim(None, metronome=float("nan")), "metronome"),
           (lambda: ctx.batch_set_trim([0.5, 0.5]), "2 chain gains"), (lambda: ctx.batch_set_trim([0.5] * 4), "4 chain gains")]
    for call, names in bad:
        with pytest.raises(pkg.GdgError, match=names) as e:
            call()
        assert e.value.code == pkg.GDG_ERR_INVALID
    metas = [(SAMPLES, "lpcm16", RATE)] * NCH
    assert ctx.batch_stream_open(metas, RATE, "lpcm16", **KW) == BLOCKS * BLOCK
    with pytest.raises(pkg.GdgError, match="open") as e:
        ctx.batch_set_trim([2.0, 2.0, 2.0])                                 # configuration does not change under an open job
    assert e.value.code == pkg.GDG_ERR_INVALID
    ctx.batch_stream_close()
    got = ctx.batch_run(job.inputs, RATE, "lpcm16", **KW)                   # a fresh context's run: nothing has been processed on it yet
    ctx.close()
    for r in range(NCH + 3):
        assert np.array_equal(got[r], want[r]), r


# ---- 7: the two-pass helper --------------------------------------------------------------------------------------------------------------
def test_render_normalized_brings_three_rigs_of_very_different_level_to_the_target():
    import __graft_entry__ as entry
    entry.load_package()                                                    # build() has made both libraries
    from go_dsp_guitar_amd import host
    nch, S = 3, ref.SCALE["lpcm24"]
    irs = host.ImpulseResponses()
    irs.add("Cab", RATE, -20, synth_ir(500, seed=3))
    eng = host.Engine(nch, BLOCK)
    for c in range(nch):
        ch = eng.create_chain(irs)
        ch.SetBypass(ch.AppendUnit(19), False)                              # a power amp
        ch.SetDiscreteValue(0, "filter_1", "Cab")
    sp = host.Spatializer(eng, nch)
    sp.SetSampleRate(RATE)
    for c in range(nch):
        sp.SetAzimuth(c, -50.0 + 50.0 * c); sp.SetDistance(c, 1.0 + 0.5 * c); sp.SetLevel(c, 0.9)
    inputs = [(lpcm16_file(level * synth_signal(c, SAMPLES, RATE)), "lpcm16", RATE) for c, level in enumerate((0.9, 0.03, 0.0008))]
    target = 10.0 ** (-1.0 / 20.0)
    outs, gains = eng.render_normalized(-1.0, 40.0, inputs, RATE, "lpcm24", window=2)
    assert eng.last_error() == ""
    tp, report = eng.normalize_true_peak, eng.normalize_report
    assert tp.shape == (nch + 3, BLOCKS) and report.shape == (nch + 3, BLOCKS)
    assert np.array_equal(gains, ref.plan(tp["true_peak"], target, 100.0))
    assert gains[nch + 2] == 1.0 and gains[0] < gains[1] <= gains[2] == 100.0                # the silent metronome; the order of the levels; the cap
    for r in range(nch + 3):
        peak = report["peak"][r].max()
        assert peak <= tp["true_peak"][r].max()
        biggest = int(np.abs(dither_ref.decode_codes("lpcm24", outs[r])).max())
        assert biggest == int(np.trunc(S * min(abs(gains[r]) * peak, 1.0))), (r, gains[r], peak, biggest)
        if gains[r] < 100.0 and peak > 0.0:
            assert 0 < biggest <= int(np.trunc(S * target))                                     # |g| * true_peak <= target: nothing above it
    del sp
    eng.close()
