"""The loudness records (include/gdg.h, LOUDNESS) on the device: the stand-alone call against the recurrence run sequentially in
np.longdouble (tests/loudness_ref.py) at every length at which the kernel takes another path, a stream continued through the state, and a
batch job whose hops are the same 64 bits whatever the window, however the job is sliced, with and without outputs and on the job's own
float64 rows; off; what is refused; and two rigs of different gain brought to one loudness."""
import math
import zlib

import numpy as np
import pytest

import loudness_ref as ref
from helpers import package, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
LENGTHS = [1, 31, 32, 33, 4409, 4410, 4411, 8191, 8192, 8193, 19201, 3 * 8192 + 5]
RATES = [44100, 48000, 192000]
SIGNALS = ["noise", "sine 40 Hz", "sine 10 kHz", "impulse", "silence", "NaN and inf", "subnormal"]
BAR = 1e-9                                                                  # the project's parity bar, relative to the hop's value


@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


def signals(rate, n):
    rng = np.random.default_rng(0x10d)
    t = np.arange(n)
    x = np.zeros((len(SIGNALS), n))
    x[0] = rng.uniform(-1.0, 1.0, n)
    x[1] = np.sin(2 * np.pi * 40.0 * t / rate)
    x[2] = 0.5 * np.sin(2 * np.pi * 10000.0 * t / rate)
    x[3, 3] = 1.0
    x[5] = rng.uniform(-0.5, 0.5, n)
    x[5, 300] = np.nan
    x[5, 5000] = np.inf
    x[5, 8191] = -np.inf
    x[6] = rng.uniform(-1.0, 1.0, n) * 1e-310
    return x


# ---- 1: the stand-alone call ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
def test_every_length_against_the_longdouble_reference(ctx1, rate):
    """rows of 1 and of 3, every length, every signal: each emitted hop within 1e-9 of its value; a hop whose reference is 0 reads +0.0"""
    n = LENGTHS[-1]
    x = signals(rate, n)
    want = np.stack([ref.hop_sums(y, rate, exact=True) for y in ref.k_weight_rows_longdouble(x, rate)])      # [signals][hops] in longdouble
    plain = np.stack([ref.hop_sums(ref.k_weight(r, rate), rate, exact=True) for r in x])
    assert want.shape == (len(SIGNALS), ref.hops(rate, 0, n)) and (want[4] == 0).all() and (want[6] == 0).all() and (want[0] > 0).all()

    worst = {s: 0.0 for s in SIGNALS}

    def deviations(got, rows, hops):
        for i, r in enumerate(rows):
            for h in range(hops):
                w = want[r, h]
                if w == 0:
                    assert got[i, h] == 0.0 and not np.signbit(got[i, h]), (rate, SIGNALS[r], h, got[i, h])
                else:
                    worst[SIGNALS[r]] = max(worst[SIGNALS[r]], float(abs(np.longdouble(got[i, h]) - w) / w))

    for length in LENGTHS:
        hops = ref.hops(rate, 0, length)
        assert package().loudness_hops(rate, 0, length) == hops
        for rows in [[r] for r in range(len(SIGNALS))] + [[0, 1, 2], [3, 4, 5], [6, 5, 0]]:
            got, state = ctx1.loudness_rows(x[rows, :length], rate)
            assert got.shape == (len(rows), hops) and state.shape == (len(rows), ref.STATE_DOUBLES) and (state[:, 6] == length).all()
            deviations(got, rows, hops)
    yard = max(float(abs(plain[r, h] - want[r, h]) / want[r, h]) for r in range(len(SIGNALS)) for h in range(want.shape[1]) if want[r, h] != 0)
    print("rate %d: largest deviation from the longdouble reference per signal %s; the float64 sequential restatement's own: %.3e" % (
        rate, {s: "%.3e" % v for s, v in worst.items()}, yard))
    assert max(worst.values()) <= BAR, worst


def test_a_stream_continued_through_the_state_has_the_bits_of_the_one_call(ctx1):
    pkg = package()
    rate, n = 44100, 5 * BLOCK + 100
    x = signals(rate, n)[[0, 1, 5]]
    whole, end = ctx1.loudness_rows(x, rate)
    assert whole.shape == (3, ref.hops(rate, 0, n)) and (whole > 0).all()
    pieces, state = [], None
    for first in range(0, n, BLOCK):                                         # cut at every multiple of 8192, the state carried
        rec, state = ctx1.loudness_rows(x[:, first:first + BLOCK], rate, first, state)
        assert rec.shape[1] == ref.hops(rate, first, min(BLOCK, n - first))
        pieces.append(rec)
    assert np.concatenate(pieces, axis=1).tobytes() == whole.tobytes() and state.tobytes() == end.tobytes()
    for cut in range(BLOCK, n, BLOCK):                                       # ... and in two calls at each of them
        a, state = ctx1.loudness_rows(x[:, :cut], rate)
        b, state = ctx1.loudness_rows(x[:, cut:], rate, cut, state)
        assert np.concatenate([a, b], axis=1).tobytes() == whole.tobytes() and state.tobytes() == end.tobytes(), cut
    _, state = ctx1.loudness_rows(x[:, :BLOCK], rate)
    for first, text in ((BLOCK + 100, "multiple of 8192"), (2 * BLOCK, "stands at sample 8192")):
        with pytest.raises(pkg.GdgError, match="loudness rows.*" + text) as e:
            ctx1.loudness_rows(x[:, BLOCK:2 * BLOCK], rate, first, state)
        assert e.value.code == pkg.GDG_ERR_INVALID
    with pytest.raises(pkg.GdgError, match="loudness rows.*starts at sample 0"):
        ctx1.loudness_rows(x[:, :BLOCK], rate, BLOCK)
    with pytest.raises(pkg.GdgError, match="loudness rows: rate 44101") as e:
        ctx1.loudness_rows(x[:, :BLOCK], 44101)
    assert e.value.code == pkg.GDG_ERR_INVALID


# ---- 2: the batch job ----------------------------------------------------------------------------------------------------------------------
NCH, BLOCKS, RATE = 4, 12, 48000
KW = dict(metronome_to_master=True)
BLENDS = [[(0, 0.6), (1, -0.4)]]
NP = NCH + 3 + len(BLENDS)
HOPS = 20


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


def crc(outs):
    c = 0
    for o in outs:
        c = zlib.crc32(o.tobytes(), c)
    return c


class Job:
    """4 channels and one blend, 11 * 8192 + 1000 samples at 48000: 12 blocks, 20 whole hops; quiet enough that no encoder clips"""

    def __init__(self):
        self.pkg = package()
        samples = (BLOCKS - 1) * BLOCK + 1000
        self.inputs = [(lpcm16_file(0.1 * synth_signal(c, samples, RATE)), "lpcm16", RATE) for c in range(NCH)]
        self.metas = [(samples, "lpcm16", RATE)] * NCH

    def configured(self, window=4, loudness=True, blends=True):
        ctx = self.pkg.Context(NCH, BLOCK)
        ctx.append_unit(0, "overdrive", params=[0, 20, 100, 0, 1, 2])
        ctx.append_unit(1, "tone_stack")
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(NCH):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * c, 1.0 + 0.5 * c, 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.2, 0.2, 800), np.linspace(0.1, -0.1, 500))
        ctx.metronome_configure(4, 150, RATE)
        ctx.set_window(window)
        if blends:
            ctx.batch_set_blends(BLENDS)
        if loudness:
            ctx.batch_loudness_enable()
        return ctx


@pytest.fixture(scope="module")
def job():
    return Job()


@pytest.fixture(scope="module")
def never(job):
    """the job on a context that never heard of the switch: its files, twice (a context's second job continues its units' state)"""
    ctx = job.configured(loudness=False)
    first = ctx.batch_run(job.inputs, RATE, "ieee64", **KW)
    second = ctx.batch_run(job.inputs, RATE, "ieee64", **KW)
    kib = ctx.get_option("stat_batch_device_kib")
    with pytest.raises(job.pkg.GdgError, match="no loudness records.*gdg_batch_loudness_enable comes before the call"):
        ctx.batch_loudness()
    ctx.close()
    return first, second, kib


def test_the_hops_do_not_depend_on_window_slices_or_outputs(job, never, ctx1):
    assert ref.hops(RATE, 0, BLOCKS * BLOCK) == HOPS
    want = None
    for window in (1, 4, 16):
        ctx = job.configured(window=window)
        outs = ctx.batch_run(job.inputs, RATE, "ieee64", **KW)
        got = ctx.batch_loudness()
        ctx.close()
        assert got.shape == (NP, HOPS) and (got >= 0).all() and got.max(axis=1).min() > 0, window      # no port is silent throughout
        assert crc(outs) == crc(never[0]), window                            # every file byte-equal to the job with the switch never touched
        if want is None:
            want = got.tobytes()
            # ... and the stand-alone call on the float64 rows of the same job
            rows = np.stack([o.view(np.float64) for o in outs])
            assert rows.shape == (NP, BLOCKS * BLOCK) and np.abs(rows).max() < 1.0
            alone, _ = ctx1.loudness_rows(rows, RATE)
            assert alone.tobytes() == want
        assert got.tobytes() == want, window
    for per_slice in (1, 2, 3, 5):
        ctx = job.configured()
        pieces, done = [], 0
        for _ in ctx.batch_stream(job.inputs, RATE, "ieee64", lambda left: min(per_slice, left), **KW):
            pieces.append(ctx.batch_loudness())
            blocks = min(per_slice, BLOCKS - done)
            assert pieces[-1].shape == (NP, ref.hops(RATE, done * BLOCK, blocks * BLOCK))
            done += blocks
        ctx.close()
        assert np.concatenate(pieces, axis=1).tobytes() == want, per_slice
    ctx = job.configured()
    assert ctx.batch_run(job.inputs, RATE, "ieee64", skip_outputs=True, **KW) is None
    assert ctx.batch_loudness().tobytes() == want
    ctx.close()


def test_off_is_off_and_every_refusal_names_the_switch(job, never):
    pkg = job.pkg
    first, second, kib = never
    ctx = job.configured(blends=True)
    on = ctx.batch_run(job.inputs, RATE, "ieee64", **KW)
    assert ctx.get_option("stat_batch_device_kib") > kib and crc(on) == crc(first)
    ctx.batch_loudness_enable(False)
    off = ctx.batch_run(job.inputs, RATE, "ieee64", **KW)
    assert ctx.get_option("stat_batch_device_kib") == kib > 0 and crc(off) == crc(second) != crc(first)
    with pytest.raises(pkg.GdgError, match="no loudness records"):
        ctx.batch_loudness()
    ctx.close()

    ctx = job.configured(blends=False)
    half = np.zeros(BLOCK)
    calls = {
        "gdg_batch_run_shard": lambda: ctx.batch_run_shard(job.inputs, RATE, "lpcm16"),
        "gdg_batch_stream_open_shard": lambda: ctx.batch_stream_open_shard(job.metas, RATE, "lpcm16"),
        "gdg_batch_finish_master:": lambda: ctx.batch_finish_master("lpcm16", [half], [half]),
        "gdg_batch_finish_master_slice": lambda: ctx.batch_finish_master_slice("lpcm16", [half], [half]),
    }
    for name, call in calls.items():
        with pytest.raises(pkg.GdgError, match=name + ".*gdg_batch_loudness_enable") as e:
            call()
        assert e.value.code == pkg.GDG_ERR_UNSUPPORTED, name
    ctx.batch_stream_open(job.metas, RATE, "lpcm16", **KW)
    with pytest.raises(pkg.GdgError, match="gdg_batch_loudness_enable: a streamed batch run is open") as e:
        ctx.batch_loudness_enable(False)
    assert e.value.code == pkg.GDG_ERR_INVALID
    with pytest.raises(pkg.GdgError, match="checkpoint.*gdg_batch_loudness_enable.*version-1") as e:
        ctx.batch_stream_checkpoint()
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    ctx.batch_stream_close()
    with pytest.raises(pkg.GdgError, match="resume.*gdg_batch_loudness_enable") as e:
        ctx.batch_stream_resume(job.metas, RATE, "lpcm16", b"\0" * 64, **KW)
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    plain = job.configured(loudness=False, blends=False)
    want = plain.batch_run(job.inputs, RATE, "ieee64", **KW)
    plain.close()
    after = ctx.batch_run(job.inputs, RATE, "ieee64", **KW)                    # after all of them: a plain job, the same bytes
    assert crc(after) == crc(want) and ctx.batch_loudness().shape == (NCH + 3, HOPS)
    ctx.close()


# ---- 3: two rigs brought to one loudness ---------------------------------------------------------------------------------------------------
def test_render_normalized_by_loudness_meets_the_target():
    """two rigs of different gain and one with large peaks: the written files, decoded and measured by the reference, read -23.0 +- 0.1 LU;
    the rig with the peaks is capped at the ceiling and reported so"""
    import __graft_entry__ as entry
    entry.load_package()
    from go_dsp_guitar_amd import host
    nch, rate, seconds = 3, 48000, 4
    blocks = -(-seconds * rate // BLOCK)
    n = np.arange(seconds * rate)
    tone = np.sin(2 * np.pi * 440.0 * n / rate) + 0.5 * np.sin(2 * np.pi * 1200.0 * n / rate)
    clicks = np.zeros(n.size)
    clicks[::4800] = 0.9                                                     # large peaks, little loudness
    inputs = [(lpcm16_file(0.4 * tone), "lpcm16", rate), (lpcm16_file(0.05 * tone), "lpcm16", rate), (lpcm16_file(clicks + 0.002 * tone), "lpcm16", rate)]
    eng = host.Engine(nch, BLOCK)
    chains = [eng.create_chain(host.ImpulseResponses()) for _ in range(nch)]
    sp = host.Spatializer(eng, nch)
    sp.SetSampleRate(rate)
    for c in range(nch):
        sp.SetAzimuth(c, -30.0 + 30.0 * c); sp.SetDistance(c, 1.0); sp.SetLevel(c, 0.9)
    outs, gains = eng.render_normalized(-1.0, 60.0, inputs, rate, "ieee64", window=4, measure="loudness", target_lufs=-23.0, ceiling_dbtp=-1.0)
    assert eng.last_error() == ""
    rows = np.stack([o.view(np.float64) for o in outs])
    assert rows.shape == (nch + 3, blocks * BLOCK)
    capped = eng.normalize_capped
    assert capped.shape == (nch + 3,) and not capped[0] and not capped[1] and capped[2]
    levels = []
    for r in range(nch):
        levels.append(ref.from_hops(ref.hop_sums(ref.k_weight(rows[r], rate), rate)[None, :], rate, [0])[0])
    print("written files read", levels, "LUFS; gains", gains, "capped", capped)
    assert abs(levels[0] + 23.0) <= 0.1 and abs(levels[1] + 23.0) <= 0.1
    assert levels[2] < -23.1 and abs(np.abs(rows[2]).max() - 10.0 ** (-1.0 / 20.0)) < 0.02      # at the ceiling, not at the target
    assert gains[1] / gains[0] == pytest.approx(8.0, rel=0.02)
    assert math.isfinite(gains[2])
    del chains, sp
