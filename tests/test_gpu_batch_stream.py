"""The streamed batch run (gdg_batch_stream_open / _need / _step / _close): the job of gdg_batch_run fed and drained in slices of whole
8192-sample blocks.  The yardstick is the one-call gdg_batch_run on a fresh, identically configured context -- every output byte for
byte, float containers included: same kernels, same order -- and beside it the oracle pipeline."""
import numpy as np
import pytest

from helpers import TOL_RMS, ChainPair, package, rms, synth_ir, synth_signal
from test_gpu_fuzz import random_params

pytestmark = pytest.mark.gpu

BLOCK = 8192
FORMATS = ["lpcm8", "lpcm16", "lpcm24", "lpcm32", "ieee32", "ieee64"]
CHAIN = [("compressor", [1, 30, -20]), ("overdrive", [0, 15, 80, -3, 1, 0]), ("tone_stack", None), ("chorus", None),
         ("power_amp", "ir"), ("cabinet", None), ("reverb", [30])]


def stream(ctx, inputs, rate, out_fmt, slicing, **kw):
    """the job in the slices of `slicing` (block counts); returns the N + 3 outputs joined"""
    it = iter(slicing)
    parts = list(ctx.batch_stream(inputs, rate, out_fmt, lambda left: next(it), **kw))
    wo = pkg_width(out_fmt)
    assert [[o.size for o in p] for p in parts] == [[k * BLOCK * wo] * len(inputs + [0, 0, 0]) for k in slicing]
    return [np.concatenate([p[r] for p in parts]) for r in range(len(parts[0]))]


def pkg_width(fmt):
    pkg = package()
    return pkg.lib().gdg_wave_bytes_per_sample(pkg.WAVE_FORMATS[fmt])


def random_slicing(rng, blocks, most=16):
    cuts, left = [], blocks
    while left:
        k = int(min(left, rng.integers(1, most + 1)))
        cuts.append(k)
        left -= k
    return cuts


def encode_file(oracle, pkg, fmt, chan_samples):
    """interleaved frames (wave.go:237-270) of the given channels"""
    w = pkg.lib().gdg_wave_bytes_per_sample(pkg.WAVE_FORMATS[fmt])
    n = len(chan_samples[0])
    per_chan = [oracle.wave_encode(fmt, s).reshape(n, w) for s in chan_samples]
    return np.ascontiguousarray(np.stack(per_chan, axis=1)).reshape(-1)


def _batch_case(oracle, pkg):
    """A small batch with every special case of controller.processFiles (controller.go:2809-3219) and its oracle result: a stereo file
    whose second channel is taken and whose rate already is the target (no resampling, :2993), an empty input (:2935), inputs at two
    other rates, the metronome in the master mix (metrMasterOutput), meters on, tuner fed."""
    rate, nch = 48000, 5
    rng = np.random.default_rng(11)
    irs = [synth_ir(2000, seed=40 + c) for c in range(nch)]
    positions = [(float(rng.uniform(-90, 90)), float(rng.uniform(0.3, 5)), float(rng.uniform(0.2, 1))) for _ in range(nch)]
    tick, tock = rng.uniform(-0.5, 0.5, 900), rng.uniform(-0.5, 0.5, 500)
    ports = 2 * nch + 3
    # channel: (format, rate, samples, file channels, channel taken) -- channel 3 stays empty
    files = {0: ("lpcm16", 48000, 20000, 2, 1), 1: ("lpcm24", 44100, 62000, 1, 0), 2: ("ieee32", 96000, 50000, 3, 2), 4: ("lpcm32", 48000, 9000, 1, 0)}
    inputs, decoded = [None] * nch, {}
    for c, (fmt, r, n, chans, take) in files.items():
        chan_samples = [0.7 * synth_signal(10 * c + k, n, r) for k in range(chans)]
        w = pkg.lib().gdg_wave_bytes_per_sample(pkg.WAVE_FORMATS[fmt])
        per_chan = [oracle.wave_encode(fmt, s).reshape(n, w) for s in chan_samples]
        data = np.ascontiguousarray(np.stack(per_chan, axis=1)).reshape(-1)           # interleaved frames (wave.go:237-270)
        inputs[c] = (data, fmt, r, chans, take)
        x = oracle.wave_decode(fmt, per_chan[take].reshape(-1))
        decoded[c] = x if r == rate else oracle.resample_time(x, r, rate)
    longest = max(len(x) for x in decoded.values())
    length = BLOCK * ((longest + BLOCK - 1) // BLOCK)
    ref_in = np.zeros((nch, length))
    for c, x in decoded.items():
        ref_in[c, :len(x)] = x

    # ---- oracle ---------------------------------------------------------------------------------------------------------
    chains = []
    for c in range(nch):
        ch = oracle.Chain()
        for name, p in CHAIN:
            ch.append_unit(name, fir=irs[c]) if p == "ir" else ch.append_unit(name, params=p)
        chains.append(ch)
    ref_sp = oracle.Spatializer(nch)
    ref_sp.set_sample_rate(rate)
    for c, (a, d, l) in enumerate(positions):
        ref_sp.set_azimuth(c, a); ref_sp.set_distance(c, d); ref_sp.set_level(c, l)
    ref_met = oracle.Metronome()
    ref_met.tick, ref_met.tock = tick, tock
    ref_met.s.beats_per_period, ref_met.s.bpm_speed, ref_met.s.sample_rate = 3, 200, rate
    ref_meters = [oracle.ChannelMeter() for _ in range(ports)]
    for m in ref_meters:
        m.set_enabled(True)
    ref_tuners = [oracle.Tuner() for _ in range(nch)]
    ref_out = np.zeros((nch + 3, length))
    for b in range(length // BLOCK):
        sl = slice(b * BLOCK, (b + 1) * BLOCK)
        for c in range(nch):
            ref_tuners[c].process(ref_in[c, sl], rate)
            ref_out[c, sl] = chains[c].process(ref_in[c, sl], rate)
        ref_out[nch + 2, sl] = ref_met.process(BLOCK)
        ref_out[nch, sl], ref_out[nch + 1, sl] = ref_sp.process(ref_out[:nch, sl], aux=ref_out[nch + 2, sl])
        rows = [ref_in[c, sl] for c in range(nch)] + [ref_out[c, sl] for c in range(nch)] + [ref_out[nch + 2, sl], ref_out[nch, sl], ref_out[nch + 1, sl]]
        for m, r in zip(ref_meters, rows):
            m.process(r, rate)

    def configured(first=0, count=nch):
        """a context carrying channels first .. first + count - 1 of the job (the whole job by default)"""
        ctx = pkg.Context(count, BLOCK)
        for c in range(count):
            for name, p in CHAIN:
                ctx.append_unit(c, name, fir=irs[first + c]) if p == "ir" else ctx.append_unit(c, name, params=p)
        ctx.spatializer_set_sample_rate(rate)
        for c in range(count):
            ctx.spatializer_set_position(c, *positions[first + c])
        ctx.metronome_set_sounds(tick, tock)
        ctx.metronome_configure(3, 200, rate)
        ctx.meter_configure(2 * count + 3)
        ctx.meter_set_enabled(True)
        return ctx

    assert length == 9 * BLOCK
    from types import SimpleNamespace
    return SimpleNamespace(rate=rate, nch=nch, inputs=inputs, length=length, ref_out=ref_out, ref_meters=ref_meters, ref_tuners=ref_tuners,
                           configured=configured)

_case = {}


def batch_case(oracle):
    if "case" not in _case:
        _case["case"] = _batch_case(oracle, package())
    return _case["case"]


def after_job(ctx):
    lv, pk = ctx.meter_analyze()
    return [int(v) for v in lv], [int(v) for v in pk], ctx.tuner_analyze(), bytes(ctx.save_state())


def same_tuners(a, b):
    for x, y in zip(a, b):
        assert x["note_index"] == y["note_index"] and x["cents"] == y["cents"]
        assert x["frequency"] == y["frequency"] or (np.isnan(x["frequency"]) and np.isnan(y["frequency"]))


@pytest.mark.parametrize("W", [1, 2, 8])
@pytest.mark.parametrize("out_fmt", ["lpcm24", "ieee64"])
def test_sliced_job_has_the_bytes_of_the_one_call_run(oracle, out_fmt, W):
    """The job of tests/test_gpu_end_to_end.py's _batch_case (stereo pick, empty input, 44.1 and 96 kHz into 48 kHz, metronome in the master,
    meters, tuner) in four slicings: outputs, meters, tuner results and the saved state equal the one-call context's; and the one-call
    test's own assertions against the oracle."""
    case = batch_case(oracle)
    rate, nch, inputs, length, ref_out = case.rate, case.nch, case.inputs, case.length, case.ref_out
    kw = dict(metronome_to_master=True, run_meters=True, tuner_enqueue=True)
    ctx = case.configured()
    ctx.set_window(W)
    want = ctx.batch_run(inputs, rate, out_fmt, **kw)
    want_after = after_job(ctx)
    ctx.close()
    for slicing in ([1] * 9, [4, 4, 1], [1, 8], [9]):
        ctx = case.configured()
        ctx.set_window(W)
        outs = stream(ctx, inputs, rate, out_fmt, slicing, **kw)
        got_after = after_job(ctx)
        ctx.close()
        assert len(outs) == nch + 3
        for r in range(nch + 3):
            assert np.array_equal(outs[r], want[r]), "output %d, slices %s, W = %d" % (r, slicing, W)
        assert got_after[0] == want_after[0] and got_after[1] == want_after[1], slicing
        same_tuners(got_after[2], want_after[2])
        assert got_after[3] == want_after[3], "saved state, slices %s" % (slicing,)
        # the oracle, as test_batch_run_one_call_matches_oracle asks
        for r in range(nch + 3):
            ref = oracle.wave_encode(out_fmt, ref_out[r])
            assert outs[r].size == ref.size == length * (8 if out_fmt == "ieee64" else 3)
            if out_fmt == "ieee64":
                err = rms(outs[r].view(np.float64) - ref_out[r])
                assert err <= TOL_RMS, "output %d: RMS %.3e" % (r, err)
            else:
                np.testing.assert_array_equal(outs[r], ref, err_msg="output %d" % r)
        for p, m in enumerate(case.ref_meters):
            assert (got_after[0][p], got_after[1][p]) == m.analyze(), "meter port %d" % p
        for c in range(nch):
            ref = case.ref_tuners[c].analyze()
            got = got_after[2][c]
            assert got["note_index"] == ref["note_index"] and got["cents"] == ref["cents"], (c, got, ref)
            if np.isnan(ref["frequency"]):
                assert np.isnan(got["frequency"])
            else:
                assert abs(got["frequency"] - ref["frequency"]) <= 1e-9 * max(1.0, abs(ref["frequency"]))


def shard_run_with_encoded_metronome_only(ctx, inputs, rate, out_fmt, job_samples, **kw):
    """gdg_batch_run_shard with the encoded metronome track asked for and the float64 one not: (outs, left, right, metronome_bytes)"""
    import ctypes as C
    pkg = package()
    n = len(inputs)
    arr, _keep = ctx._batch_inputs(inputs)
    fo = pkg.WAVE_FORMATS[out_fmt]
    wo = pkg_width(out_fmt)
    opt = pkg.BatchOptions(rate, fo, 0, int(kw.get("run_meters", False)), int(kw.get("tuner_enqueue", False)))
    outs = [np.zeros(job_samples * wo, dtype=np.uint8) for _ in range(n)]
    left, right, mb = np.zeros(job_samples), np.zeros(job_samples), np.zeros(job_samples * wo, dtype=np.uint8)
    ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    so = pkg.BatchShardOut(left.ctypes.data, right.ctypes.data, mb.ctypes.data, None, job_samples)
    ctx._check(pkg.lib().gdg_batch_run_shard(ctx._h, arr, n, C.byref(opt), ptrs, C.byref(so)))
    return outs, left, right, mb


def test_one_call_runs_between_a_streamed_and_a_shard_job_on_one_context(oracle):
    """The one-call run is the single slice of a job of its own.  One context, no batch_release in between: a one-call run, the same job
    streamed in slices [4, 4, 1], a one-call shard run (job_samples one block longer than its files need, only the encoded metronome
    track asked for) and the one-call run again.  Everything the first and the last run leave -- outputs, meters, tuner, saved state --
    equals, byte for byte, a fresh context's that did the same four jobs through batch_run / batch_run_shard only: the six device buffers
    serve all three kinds of run, the one-call run's job never becomes the context's, and a shard's rows fit the room its job sized."""
    pkg = package()
    case = batch_case(oracle)
    rate, nch, inputs, length = case.rate, case.nch, case.inputs, case.length
    out_fmt, kw = "lpcm24", dict(run_meters=True, tuner_enqueue=True)
    not_open = "no streamed batch run is open"

    def one_call(ctx):
        outs = ctx.batch_run(inputs, rate, out_fmt, metronome_to_master=True, **kw)
        with pytest.raises(pkg.GdgError, match=not_open):        # the job it ran was its own: the context's stayed closed
            ctx.batch_stream_need(1)
        return outs, after_job(ctx)

    def sequence(streamed):
        ctx = case.configured()
        ctx.set_window(2)
        first = one_call(ctx)
        if streamed:
            parts = []
            slicing = iter([4, 4, 1])
            for part in ctx.batch_stream(inputs, rate, out_fmt, lambda left: next(slicing), metronome_to_master=True, **kw):
                parts.append(part)
                if len(parts) == 1:                              # a one-call run while the job is open: refused, and the job goes on
                    for run in (ctx.batch_run, ctx.batch_run_shard):
                        with pytest.raises(pkg.GdgError, match="a streamed batch run is open on this context: gdg_batch_stream_close it first") as e:
                            run(inputs, rate, out_fmt)
                        assert e.value.code == pkg.GDG_ERR_INVALID
                    assert len(ctx.batch_stream_need(4)) == nch
            assert [p[0].size for p in parts] == [4 * BLOCK * 3, 4 * BLOCK * 3, BLOCK * 3]
            second = [np.concatenate([p[r] for p in parts]) for r in range(nch + 3)]
        else:
            second = ctx.batch_run(inputs, rate, out_fmt, metronome_to_master=True, **kw)
        shard = shard_run_with_encoded_metronome_only(ctx, inputs, rate, out_fmt, length + BLOCK, **kw)
        with pytest.raises(pkg.GdgError, match=not_open):
            ctx.batch_stream_need(1)
        last = one_call(ctx)
        assert ctx.get_option("stat_batch_device_kib") > 0
        ctx.close()
        return first, second, shard, last

    got, want = sequence(True), sequence(False)
    for name, g, w in (("first", got[0], want[0]), ("last", got[3], want[3])):
        for r in range(nch + 3):
            assert np.array_equal(g[0][r], w[0][r]), "%s run, output %d" % (name, r)
        assert g[1][0] == w[1][0] and g[1][1] == w[1][1], "%s run: meters" % name
        same_tuners(g[1][2], w[1][2])
        assert g[1][3] == w[1][3], "%s run: saved state" % name
    for r in range(nch + 3):
        assert np.array_equal(got[1][r], want[1][r]), "streamed job, output %d" % r
    for g, w in zip(got[2][0] + list(got[2][1:]), want[2][0] + list(want[2][1:])):
        assert np.array_equal(g, w), "shard job"
    assert got[2][3].any()                                       # the encoded metronome track came down


@pytest.mark.parametrize("rate", [48000, 44100])
def test_resampler_across_slices_has_the_bits_of_the_whole_file(oracle, rate):
    """resample.Time alone: every container format as input, rates up and down, files longer than three slices and one shorter than a
    block, chains empty, float64 out.  Every cut between slices falls inside a Lanczos window of every resampled input (checked): a
    contraction, a reordering or an off-by-one in the frames kept from slice to slice shows here."""
    pkg = package()
    sources = [44100, 96000, 22050, 192000, 47999, 8000, 88200, 48000, 32000, 11025, 96000, 44100]
    sources = [s if s != rate else 37800 for s in sources]
    files = []
    for c, src in enumerate(sources):
        fmt = FORMATS[c % 6]
        chans = 1 + (c % 3 == 1)                                 # some interleaved: the pick and the resampler together
        n_target = [7 * BLOCK + 100 * c + 13, 5 * BLOCK - 7, 6 * BLOCK + 1][c % 3] if c != 5 else 3000
        n = max(8, int(n_target * src / rate))
        chan_samples = [0.8 * synth_signal(3 * c + k, n, src) for k in range(chans)]
        files.append((encode_file(oracle, pkg, fmt, chan_samples), fmt, src, chans, chans - 1, n))
    nch = len(files)
    inputs = [f[:5] for f in files]
    ctx = pkg.Context(nch, BLOCK)
    want = ctx.batch_run(inputs, rate, "ieee64")
    length = want[0].size // 8
    assert length >= 7 * BLOCK
    whole = []
    for data, fmt, src, chans, take, n in files:
        x = ctx.wave_decode(fmt, data, channels=chans)
        x = x if chans == 1 else x[take]
        whole.append(ctx.resample_time(np.ascontiguousarray(x), src, rate))
    ctx.close()
    assert min(len(w) for w in whole) < BLOCK                    # one file shorter than a block
    for W, slicing in ((1, [2] * (length // BLOCK // 2) + [1] * (length // BLOCK % 2)), (2, [1] * (length // BLOCK)), (4, [3, 1, 2] + [1] * (length // BLOCK - 6)),
                       (8, [length // BLOCK])):
        assert sum(slicing) == length // BLOCK and (len(slicing) > 3 or W == 8)
        pos = 0
        for k in slicing[:-1]:                                   # the cut behind this slice: the next slice reads frames this one brought
            pos += k * BLOCK
            for (data, fmt, src, chans, take, n), w in zip(files, whole):
                if pos < len(w):
                    before = pkg.batch_stream_span(n, src, rate, pos - 1, 1)
                    after = pkg.batch_stream_span(n, src, rate, pos, 1)
                    assert after[0] < before[0] + before[1], "the cut at %d is not inside a window of a %d Hz input" % (pos, src)
        ctx = pkg.Context(nch, BLOCK)
        ctx.set_window(W)
        outs = stream(ctx, inputs, rate, "ieee64", slicing)
        ctx.close()
        for r in range(nch + 3):
            assert np.array_equal(outs[r], want[r]), "output %d, W = %d, slices %s" % (r, W, slicing)
        for c, w in enumerate(whole):
            got = outs[c].view(np.float64)
            assert np.array_equal(got[:len(w)].view(np.uint64), np.asarray(w).view(np.uint64)), "input %d (%d Hz, %s): not gdg_resample_time's bits" % (c, files[c][2], files[c][1])
            assert not got[len(w):].any()


def _long_job(oracle, pkg, blocks=41):
    rate, nch = 48000, 4
    n = blocks * BLOCK - 1234
    spec = [("lpcm16", 48000, n, 1, 0), ("lpcm24", 44100, int((n - 5000) * 44100 / 48000), 2, 1), ("ieee32", 96000, int((n - 90000) * 2), 1, 0),
            ("lpcm32", 48000, 3 * BLOCK + 17, 3, 1)]
    inputs = []
    for c, (fmt, r, m, chans, take) in enumerate(spec):
        inputs.append((encode_file(oracle, pkg, fmt, [0.7 * synth_signal(5 * c + k, m, r) for k in range(chans)]), fmt, r, chans, take))
    irs = [synth_ir(2500, seed=70 + c) for c in range(nch)]

    def configured():
        ctx = pkg.Context(nch, BLOCK)
        for c in range(nch):
            for name, p in CHAIN:
                ctx.append_unit(c, name, fir=irs[c]) if p == "ir" else ctx.append_unit(c, name, params=p)
        ctx.spatializer_set_sample_rate(rate)
        for c in range(nch):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * c, 1.0 + c, 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
        ctx.metronome_configure(4, 150, rate)
        ctx.meter_configure(2 * nch + 3)
        ctx.meter_set_enabled(True)
        return ctx
    return rate, inputs, configured


def test_a_long_job_in_random_slicings_has_the_bytes_of_the_one_call_run(oracle):
    """41 blocks, sixteen seeded slicings (slices of 1 to 16 blocks, windows of 1 to 16): one one-call run is the yardstick for all."""
    pkg = package()
    rate, inputs, configured = _long_job(oracle, pkg)
    kw = dict(metronome_to_master=True, run_meters=True, tuner_enqueue=True)
    ctx = configured()
    ctx.set_window(4)
    want = ctx.batch_run(inputs, rate, "lpcm24", **kw)
    want_after = after_job(ctx)
    ctx.close()
    blocks = want[0].size // 3 // BLOCK
    assert blocks >= 40
    for seed in range(16):
        rng = np.random.default_rng(4100 + seed)
        W = int(rng.choice([1, 2, 4, 8, 16]))
        slicing = random_slicing(rng, blocks)
        ctx = configured()
        ctx.set_window(W)
        outs = stream(ctx, inputs, rate, "lpcm24", slicing, **kw)
        got_after = after_job(ctx)
        ctx.close()
        for r in range(len(want)):
            assert np.array_equal(outs[r], want[r]), "seed %d: output %d, W = %d, slices %s" % (seed, r, W, slicing)
        # (the saved state is compared where the windows are the one-call context's, in the test above: a blob knows its context's window)
        assert got_after[0] == want_after[0] and got_after[1] == want_after[1], (seed, W, slicing)
        same_tuners(got_after[2], want_after[2])


@pytest.mark.parametrize("seed", range(16))
def test_random_streamed_jobs_follow_the_oracle_pipeline(oracle, seed):
    """The random jobs of test_gpu_fuzz.py's test_random_batch_runs_follow_the_oracle_pipeline (formats, odd lengths, rates, interleaved
    and empty inputs, random chains, window, metronome, output format), streamed in a random slicing, under that test's own rules:
    8-, 16- and 24-bit containers byte for byte except samples on a code boundary, 32-bit codes within the float tolerance, float
    containers within 1e-9 RMS."""
    pkg = package()
    rng = np.random.default_rng(7000 + seed)
    rate = int(rng.choice([44100, 48000, 96000]))
    nch = int(rng.integers(2, 6))
    W = int(rng.choice([1, 2, 4, 8]))
    out_fmt = str(rng.choice(FORMATS))
    to_master = bool(rng.random() < 0.5)
    # ---- the files ------------------------------------------------------------------------------------------------------------
    inputs, decoded = [None] * nch, {}
    for c in range(nch):
        if rng.random() < 0.15:
            continue                                             # "leaving channel empty"
        fmt = str(rng.choice(FORMATS))
        r = int(rng.choice([rate, rate, 44100, 22050]))
        n = int(rng.choice([1, 7, 5000, BLOCK, BLOCK + 1, 3 * BLOCK - 5, 20000]))
        chans = int(rng.choice([1, 1, 2, 3]))
        take = int(rng.integers(0, chans))
        w = pkg.lib().gdg_wave_bytes_per_sample(pkg.WAVE_FORMATS[fmt])
        per_chan = [oracle.wave_encode(fmt, 0.8 * synth_signal(7 * c + k, n, r)).reshape(n, w) for k in range(chans)]
        data = np.ascontiguousarray(np.stack(per_chan, axis=1)).reshape(-1)
        inputs[c] = (data, fmt, r, chans, take)
        xd = oracle.wave_decode(fmt, per_chan[take].reshape(-1))
        decoded[c] = xd if r == rate else oracle.resample_time(xd, r, rate)
    longest = max([len(v) for v in decoded.values()] + [0])
    length = BLOCK * ((longest + BLOCK - 1) // BLOCK)
    # ---- chains, spatializer, metronome on both sides ----------------------------------------------------------------------------
    ctx = pkg.Context(nch, BLOCK)
    ctx.set_window(W)
    refs = []
    for c in range(nch):
        p = ChainPair(ctx, c, oracle)
        fft = bool(rng.random() < 0.5)
        for _ in range(int(rng.integers(0, 5))):
            while True:
                t = int(rng.integers(0, 21))
                name = pkg.UNIT_NAMES[t]
                if (name == "power_amp" and not fft) or (name == "octaver" and (fft or p.handles)):      # an octaver only at the head (see _split_points)
                    continue
                break
            if name == "power_amp":
                p.append(name, fir=synth_ir(int(rng.choice([50, 3000, 12000])), seed=int(rng.integers(1, 10 ** 6))) * 0.7)
            else:
                p.append(name, params=random_params(rng, t, allow_oversampling=fft))
        refs.append(p.ref)
    ref_sp = oracle.Spatializer(nch)
    ctx.spatializer_set_sample_rate(rate)
    ref_sp.set_sample_rate(rate)
    for c in range(nch):
        a, d, l = float(rng.uniform(-180, 180)), float(rng.uniform(0.1, 10)), float(rng.uniform(0, 1))
        ctx.spatializer_set_position(c, a, d, l)
        ref_sp.set_azimuth(c, a); ref_sp.set_distance(c, d); ref_sp.set_level(c, l)
    tick, tock = rng.uniform(-0.5, 0.5, 700), rng.uniform(-0.5, 0.5, 300)
    beats, bpm = int(rng.integers(1, 8)), int(rng.integers(40, 360))
    ctx.metronome_set_sounds(tick, tock)
    ctx.metronome_configure(beats, bpm, rate)
    ref_met = oracle.Metronome()
    ref_met.tick, ref_met.tock = tick, tock
    ref_met.s.beats_per_period, ref_met.s.bpm_speed, ref_met.s.sample_rate = beats, bpm, rate
    # ---- oracle pipeline ---------------------------------------------------------------------------------------------------------
    xin = np.zeros((nch, length))
    for c, v in decoded.items():
        xin[c, :len(v)] = v
    ref_out = np.zeros((nch + 3, length))
    for b in range(length // BLOCK):
        sl = slice(b * BLOCK, (b + 1) * BLOCK)
        for c in range(nch):
            ref_out[c, sl] = refs[c].process(xin[c, sl], rate)
        ref_out[nch + 2, sl] = ref_met.process(BLOCK)
        ref_out[nch, sl], ref_out[nch + 1, sl] = ref_sp.process(ref_out[:nch, sl], aux=(ref_out[nch + 2, sl] if to_master else None))
    # ---- device: one call -----------------------------------------------------------------------------------------------------------
    # ---- device: streamed in a random slicing ---------------------------------------------------------------------------------
    slicing = random_slicing(np.random.default_rng(8000 + seed), length // BLOCK, most=3)
    outs = stream(ctx, inputs, rate, out_fmt, slicing, metronome_to_master=to_master) if length else [np.zeros(0, dtype=np.uint8)] * (nch + 3)
    ctx.close()
    wo = pkg.lib().gdg_wave_bytes_per_sample(pkg.WAVE_FORMATS[out_fmt])
    assert len(outs) == nch + 3 and all(o.size == length * wo for o in outs), (seed, [o.size for o in outs], length)
    for r in range(nch + 3):
        want = oracle.wave_encode(out_fmt, ref_out[r]) if length else np.zeros(0, dtype=np.uint8)
        if out_fmt in ("ieee32", "ieee64"):
            err = rms(oracle.wave_decode(out_fmt, outs[r]) - oracle.wave_decode(out_fmt, want)) if length else 0.0
            assert err <= TOL_RMS, (seed, r, out_fmt, err)
        elif out_fmt == "lpcm32":
            # a 32-bit code is 4.7e-10 wide: the chains' legitimate 1e-16 .. 1e-15 differences (device exp / sin / log10 against glibc's, scan
            # association) move a sample across a truncation boundary about once in 10^6 samples (seed 2056 of profiles/probes/fuzz_soak.py).
            # The encoder itself is bit exact on equal input (test_random_codec_and_resampler_jobs...): here a few codes may be off by one.
            got_i = outs[r].view("<i4").astype(np.int64) if length else np.zeros(0, dtype=np.int64)
            want_i = want.view("<i4").astype(np.int64) if length else np.zeros(0, dtype=np.int64)
            d = np.abs(got_i - want_i)
            # behind stages the reference computes by FFT (oversampled units, power amps) the float difference reaches 1e-13 and one sample in a
            # few thousand moves (seed 5421 of the soak: 10 of 24576); the bound is the float tolerance expressed in codes
            assert d.size == 0 or (d.max() <= 2 and float(np.sqrt(np.mean((d / 2147483648.0) ** 2))) <= TOL_RMS), (seed, r, int(d.max(initial=0)), int(np.count_nonzero(d)))
        else:
            if not np.array_equal(outs[r], want):
                # a sample that sits ON a code boundary may take either code: the compressor with a peak follower and a 0 dB target (or the
                # auto-yoy at full level) puts its peaks at +-1 (1 +- one ulp) -- exactly the encoder's top boundary, where 254 or 255 is a matter
                # of the last bit (soak seeds 20198, 20445).  Every differing sample must be the code of the oracle's value moved by <= 1e-9.
                g = outs[r].reshape(length, wo)
                ok = np.all(g == want.reshape(length, wo), axis=1)
                for delta in (-1e-9, 1e-9):
                    ok |= np.all(g == oracle.wave_encode(out_fmt, ref_out[r] + delta).reshape(length, wo), axis=1)
                bad = int(np.count_nonzero(~ok))
                assert bad == 0, "seed %d output %d (%s, W = %d): %d samples differ by more than a boundary case" % (seed, r, out_fmt, W, bad)


def _plain_job(oracle, pkg, nch, blocks, seed=0):
    """same-rate mono 16-bit files of `blocks` blocks (what a caller can also cut by hand), short chains"""
    rate = 48000
    inputs = [(oracle.wave_encode("lpcm16", 0.6 * synth_signal(seed + c, blocks * BLOCK, rate)), "lpcm16", rate) for c in range(nch)]

    def configured():
        ctx = pkg.Context(nch, BLOCK)
        for c in range(nch):
            ctx.append_unit(c, "compressor", params=[1, 30, -20])
            ctx.append_unit(c, "power_amp", fir=synth_ir(1500, seed=90 + c))
            ctx.append_unit(c, "delay", params=None)
        ctx.spatializer_set_sample_rate(rate)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 300), np.linspace(0.4, -0.4, 200))
        ctx.metronome_configure(4, 120, rate)
        return ctx
    return rate, inputs, configured


def test_device_memory_follows_the_slice_not_the_job(oracle):
    pkg = package()
    nch = 8
    kib = {}
    for blocks in (16, 64):
        rate, inputs, configured = _plain_job(oracle, pkg, nch, blocks)
        # half of the inputs at another rate, one interleaved: the resampler's buffers are part of the figure
        inputs = [(d, f, 44100 if c % 2 else r) for c, (d, f, r) in enumerate(inputs)]
        ctx = configured()
        ctx.set_window(4)
        assert ctx.get_option("stat_batch_device_kib") == 0
        seen = []
        for part in ctx.batch_stream(inputs, rate, "lpcm24", 4):
            seen.append(ctx.get_option("stat_batch_device_kib"))
        assert len(seen) >= blocks // 4 and seen[0] > 0
        assert all(v == seen[0] for v in seen), "the buffers grew after the first slice: %s" % seen
        kib[blocks] = seen[0]
        length = ctx.batch_length(inputs, rate)
        if blocks == 64:
            assert seen[0] * 1024 < nch * length * 8                 # what the one-call run allocates for the decoded inputs alone
        ctx.batch_release()
        assert ctx.get_option("stat_batch_device_kib") == 0
        ctx.close()
    assert kib[16] == kib[64], kib


def test_contract_of_the_streamed_run(oracle):
    pkg = package()
    nch, blocks = 3, 6
    rate, inputs, configured = _plain_job(oracle, pkg, nch, blocks)
    metas = [(blocks * BLOCK, "lpcm16", rate)] * nch
    other_rate, other_inputs, _ = _plain_job(oracle, pkg, nch, 2, seed=50)
    slice_in = lambda need: [d[0][2 * f:2 * (f + c)] for d, (f, c) in zip(inputs, need)]
    INVALID = pkg.GDG_ERR_INVALID

    def refused(fn, *a, **k):
        with pytest.raises(pkg.GdgError) as e:
            fn(*a, **k)
        assert e.value.code == INVALID and len(str(e.value)) > len("gdg error -1: "), str(e.value)

    ctx = configured()
    ctx._stream_width = 3
    canary = [np.full(BLOCK * 3, 0xAB, dtype=np.uint8) for _ in range(nch + 3)]
    refused(ctx.batch_stream_need, 1)                               # nothing open
    refused(ctx.batch_stream_step, 1, [None] * nch, canary)
    refused(ctx.batch_stream_close)
    assert ctx.batch_stream_open(metas, rate, "lpcm24") == blocks * BLOCK
    refused(ctx.batch_stream_open, metas, rate, "lpcm24")          # a second open
    refused(ctx.batch_run, other_inputs, rate, "lpcm24", outs=[np.full(2 * BLOCK * 3, 0xAB, dtype=np.uint8) for _ in range(nch + 3)])
    refused(ctx.batch_run_shard, other_inputs, rate, "lpcm24")
    refused(ctx.batch_release)
    refused(ctx.batch_stream_need, 0)
    refused(ctx.batch_stream_need, blocks + 1)                      # beyond the job's end
    refused(ctx.batch_stream_step, 1, [None] * nch, canary)         # frames asked for and not brought
    assert all((c == 0xAB).all() for c in canary)
    first = ctx.batch_stream_step(4, slice_in(ctx.batch_stream_need(4)))
    big = [np.full(3 * BLOCK * 3, 0xAB, dtype=np.uint8) for _ in range(nch + 3)]
    refused(ctx.batch_stream_step, 3, slice_in(ctx.batch_stream_need(2)), big)       # 2 blocks are left
    assert all((c == 0xAB).all() for c in big)
    need = ctx.batch_stream_need(2)
    assert need == [(4 * BLOCK, 2 * BLOCK)] * nch
    ctx.batch_stream_step(2, slice_in(need))
    refused(ctx.batch_stream_need, 1)                               # after the last block
    refused(ctx.batch_stream_step, 1, [None] * nch, canary)
    assert all((c == 0xAB).all() for c in canary)
    ctx.batch_stream_close()
    kib = ctx.get_option("stat_batch_device_kib")
    assert kib > 0
    # a second streamed job on the same context reuses the buffers
    for _ in ctx.batch_stream(inputs, rate, "lpcm24", 4):
        assert ctx.get_option("stat_batch_device_kib") == kib
    ctx.batch_release()
    assert ctx.get_option("stat_batch_device_kib") == 0
    ctx.close()

    # a job abandoned after 4 of its 6 blocks: the context goes on as after 4 blocks fed by gdg_batch_run
    ctx = configured()
    ctx.set_window(2)
    gen = ctx.batch_stream(inputs, rate, "lpcm24", 1)
    got_head = [next(gen) for _ in range(4)]
    gen.close()                                                      # closes the job
    got = ctx.batch_run(other_inputs, rate, "lpcm24")
    ctx.close()
    ctx = configured()
    ctx.set_window(2)
    want_head = ctx.batch_run([(d[:2 * 4 * BLOCK], f, r) for d, f, r in inputs], rate, "lpcm24")
    want = ctx.batch_run(other_inputs, rate, "lpcm24")
    ctx.close()
    for r in range(nch + 3):
        assert np.array_equal(np.concatenate([p[r] for p in got_head]), want_head[r]), r
        assert np.array_equal(got[r], want[r]), r
    assert first[0].size == 4 * BLOCK * 3
