"""The dithered LPCM encoders (gdg_batch_set_dither, gdg_wave_encode_dither) on the device, byte for byte against the numpy restatement of
the arithmetic include/gdg.h states (tests/dither_ref.py): the stand-alone encoder, every encoding place of the batch engine -- one-call
run, slices, a resumed checkpoint, shards with their metronome, both forms of the master finish with its cursor -- and that off is off.
The float64 rows the encoder sees come from a run of the same job on a fresh context with IEEE64 out (whose bytes ARE the rows)."""
import numpy as np
import pytest

import dither_ref as ref
from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
LPCM = ["lpcm8", "lpcm16", "lpcm24", "lpcm32"]
RATE, NCH, BLOCKS, SEED = 48000, 4, 3, 0x5eed0123456789ab
KW = dict(metronome_to_master=True)
FIXED = [ref.PORT_LEFT, ref.PORT_RIGHT, ref.PORT_METRONOME]


# ---- 1, 2: the stand-alone encoder --------------------------------------------------------------------------------------------------------
def pool(fmt, n=8192 + 64):
    """0, +-1, values beyond +-1, values within 1e-12 of the half-code boundaries, and seeded noise at -60 dBFS"""
    rng = np.random.default_rng(17)
    x = 1e-3 * rng.standard_normal(n)
    S = ref.SCALE[fmt]
    k = rng.integers(-120, 120, n)
    special = np.stack([np.zeros(n), np.ones(n), -np.ones(n), rng.uniform(1.0, 3.0, n), rng.uniform(-3.0, -1.0, n), (k + 0.5) / S,
                        (k + 0.5) / S + 1e-12, (k + 0.5) / S - 1e-12, k / S + 1e-12, k / S - 1e-12])
    for j in range(special.shape[0]):
        x[j::16] = special[j, j::16]
    return x


@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("fmt", LPCM)
def test_standalone_encoder_has_the_restatement_s_bytes(ctx1, fmt):
    x = pool(fmt)
    for n in (1, 3, 4, 5, 1027, 8192):
        for first in (0, 2 ** 32 - 3, 2 ** 40 + 1):                       # the middle one crosses 2^32 inside one call
            for port in (0, 7, 0xfffffffd):
                for off in ((0, 5, 10, 16, 23, 37) if n <= 5 else (n % 7,)):      # short calls walk over the planted values
                    seg = x[off:off + n]
                    got = ctx1.wave_encode_dither(fmt, seg, 1, SEED, port, first)
                    want = ref.encode(fmt, seg, SEED, port, first)
                    assert np.array_equal(got, want), "%s n %d first %d port %#x: %d bytes differ" % (fmt, n, first, port, np.count_nonzero(got != want))


@pytest.mark.parametrize("fmt", LPCM)
def test_device_form_takes_unaligned_buffers(ctx1, fmt):
    """input offset by 8 bytes, output by 1: everything goes one sample per thread; and the aligned form beside it"""
    pkg = package()
    lib, w = pkg.lib(), ref.WIDTH[fmt]
    x = pool(fmt)
    for n, first, port in ((1, 0, 0), (5, 2 ** 32 - 3, 7), (1027, 2 ** 40 + 1, 0xfffffffd), (8192, 2 ** 32 - 3, 7)):
        d_in, d_out = ctx1.alloc(1, n + 2), ctx1.alloc(1, (n * w + 16 + 7) // 8)
        d_in.upload(np.concatenate([[9.0], x[:n], [9.0]]))
        for in_off, out_off in ((8, 1), (0, 0), (8, 0), (0, 1)):
            d_out.upload(np.zeros(d_out.cols))
            src = np.concatenate([[9.0], x[:n]])[in_off // 8:in_off // 8 + n]
            ctx1.wave_encode_dither_device(fmt, d_in.ptr + in_off, n, d_out.ptr + out_off, 1, SEED, port, first)
            raw = np.zeros(d_out.cols * 8, dtype=np.uint8)
            ctx1._check(lib.gdg_copy_to_host(ctx1._h, raw.ctypes.data, d_out.ptr, raw.size))
            want = ref.encode(fmt, src, SEED, port, first)
            assert np.array_equal(raw[out_off:out_off + n * w], want), (fmt, n, in_off, out_off)
            assert not raw[:out_off].any() and not raw[out_off + n * w:].any(), "bytes outside the output were written"
        d_in.free()
        d_out.free()


def test_mode_0_and_ieee_formats_are_the_plain_encoder(ctx1):
    pkg = package()
    x = pool("lpcm16", 1027)
    for fmt in LPCM + ["ieee32", "ieee64"]:
        plain = ctx1.wave_encode(fmt, x)
        assert np.array_equal(ctx1.wave_encode_dither(fmt, x, 0, SEED, 7, 5), plain), fmt
        if fmt.startswith("ieee"):
            assert np.array_equal(ctx1.wave_encode_dither(fmt, x, 1, SEED, 7, 5), plain), fmt
        else:
            assert not np.array_equal(ctx1.wave_encode_dither(fmt, x, 1, SEED, 7, 5), plain), fmt
    with pytest.raises(pkg.GdgError, match="mode 2") as e:
        ctx1.wave_encode_dither("lpcm16", x, 2, SEED, 7, 5)
    assert e.value.code == pkg.GDG_ERR_INVALID


# ---- 3: dither does what it is for -------------------------------------------------------------------------------------------------------
def test_dither_keeps_a_sine_below_one_code_and_decorrelates_the_error(ctx1):
    """Properties of the definition, checked on the restatement (whose bytes the device's equal: asserted here once more on these inputs)"""
    n, S = 65536, 32767.5
    t = np.arange(n)
    s = np.sin(2 * np.pi * 1000.0 * t / 48000.0)
    x = (0.4 / S) * s
    assert not ref.decode_codes("lpcm16", ctx1.wave_encode("lpcm16", x)).any()          # the plain encoder: all-zero codes
    q = ref.codes("lpcm16", x, 12345, 7)
    assert np.array_equal(ctx1.wave_encode_dither("lpcm16", x, 1, 12345, 7, 0), ref.encode("lpcm16", x, 12345, 7))
    amp = 2.0 * np.mean(q * s)
    print("amplitude estimate %.5f LSB" % amp)
    assert abs(amp - 0.4) <= 0.05 * 0.4
    var = np.var(q - S * x)
    print("error variance %.4f LSB^2" % var)
    assert abs(var - 0.25) <= 0.01
    rng = np.random.default_rng(5)
    y = 0.5 * np.sin(2 * np.pi * 440.0 * t / 48000.0) + 0.01 * rng.standard_normal(n)
    for port in (0, 7, ref.PORT_LEFT):
        e = ref.codes("lpcm16", y, 12345, port) - S * y
        c_sig = np.corrcoef(e, y)[0, 1]
        c_lag = np.corrcoef(e[1:], e[:-1])[0, 1]
        print("port %#x: corr(error, signal) %.4f, lag-1 autocorrelation %.4f" % (port, c_sig, c_lag))
        assert abs(c_sig) < 0.02 and abs(c_lag) < 0.02


# ---- 4 .. 8: the batch engine ------------------------------------------------------------------------------------------------------------
def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """4 channels, each with overdrive and a 300-tap power amp; 3 blocks; window 2; metronome to master"""

    def __init__(self):
        self.pkg = package()
        self.inputs = [(lpcm16_file(0.6 * synth_signal(c, BLOCKS * BLOCK, RATE)), "lpcm16", RATE) for c in range(NCH)]
        self.irs = [synth_ir(300, seed=60 + c) for c in range(NCH)]
        self.cache = {}

    def configured(self, first=0, count=NCH, same_chain=False):
        ctx = self.pkg.Context(count, BLOCK)
        for c in range(count):
            ctx.append_unit(c, "overdrive", params=[0, 15, 80, -3, 1, 0])
            ctx.append_unit(c, "power_amp", fir=self.irs[0 if same_chain else first + c])
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(count):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * (first + c), 1.0 + 0.5 * (first + c), 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
        ctx.metronome_configure(4, 150, RATE)
        ctx.set_window(2)
        return ctx

    def run(self, fmt, dither, report=False):
        """the one-call run on a fresh context -> (outs, report records, stat_batch_device_kib); dither: None (never configured) or a seed"""
        key = (fmt, dither, report)
        if key not in self.cache:
            ctx = self.configured()
            if dither is not None:
                ctx.batch_set_dither(1, dither, 0)
            if report:
                ctx.batch_report_enable()
            outs = ctx.batch_run(self.inputs, RATE, fmt, **KW)
            self.cache[key] = (outs, ctx.batch_report().tobytes() if report else None, ctx.get_option("stat_batch_device_kib"))
            ctx.close()
        return self.cache[key]

    def rows(self):
        return [o.view(np.float64) for o in self.run("ieee64", None)[0]]


@pytest.fixture(scope="module")
def job():
    return Job()


def ports():
    return list(range(NCH)) + FIXED


@pytest.mark.parametrize("fmt", ["lpcm16", "lpcm24"])
def test_batch_run_writes_the_restatement_of_its_rows(job, fmt):
    rows = job.rows()
    assert len(rows) == NCH + 3 and all(r.size == BLOCKS * BLOCK and np.isfinite(r).all() and r.any() for r in rows)
    outs = job.run(fmt, SEED)[0]
    for r, port in enumerate(ports()):
        want = ref.encode(fmt, rows[r], SEED, port, 0)
        assert np.array_equal(outs[r], want), "%s, output %d (port %#x): %d bytes differ" % (fmt, r, port, np.count_nonzero(outs[r] != want))


def test_slices_and_a_resumed_checkpoint_write_the_one_call_bytes(job):
    pkg = job.pkg
    want = job.run("lpcm16", SEED)[0]
    ctx = job.configured()
    ctx.batch_set_dither(1, SEED, 0)
    it = iter([1, 2])
    parts = list(ctx.batch_stream(job.inputs, RATE, "lpcm16", lambda left: next(it), **KW))
    for r in range(NCH + 3):
        assert np.array_equal(np.concatenate([p[r] for p in parts]), want[r]), r
    ctx.close()
    # slice 1, a checkpoint, and slice 2 on a fresh context on which the dither was set again
    metas = [(BLOCKS * BLOCK, "lpcm16", RATE)] * NCH
    cut = lambda need: [d[0][2 * f:2 * (f + c)] for d, (f, c) in zip(job.inputs, need)]
    ctx = job.configured()
    ctx.batch_set_dither(1, SEED, 0)
    assert ctx.batch_stream_open(metas, RATE, "lpcm16", **KW) == BLOCKS * BLOCK
    with pytest.raises(pkg.GdgError, match="open") as e:
        ctx.batch_set_dither(1, SEED + 1, 0)                               # configuration does not change under an open job
    assert e.value.code == pkg.GDG_ERR_INVALID
    ctx.batch_dither_seek(BLOCK)                                           # the master cursor is no part of the job: it may move, and moves nothing here
    head = ctx.batch_stream_step(1, cut(ctx.batch_stream_need(1)))
    blob = ctx.batch_stream_checkpoint()
    ctx.batch_stream_close()
    ctx.close()
    ctx = job.configured()
    ctx.batch_set_dither(1, SEED, 0)
    assert ctx.batch_stream_resume(metas, RATE, "lpcm16", blob, **KW) == BLOCK
    tail = ctx.batch_stream_step(2, cut(ctx.batch_stream_need(2)))
    ctx.batch_stream_close()
    ctx.close()
    for r in range(NCH + 3):
        assert np.array_equal(np.concatenate([head[r], tail[r]]), want[r]), "resumed: output %d" % r


def test_shards_write_the_single_context_files_and_the_master_follows_its_cursor(job):
    pkg = job.pkg
    single = job.run("lpcm16", SEED)[0]
    n = BLOCKS * BLOCK
    split = [(0, 2), (2, 2)]
    ctxs = [job.configured(f, c) for f, c in split]
    for ctx, (f, _) in zip(ctxs, split):
        ctx.batch_set_dither(1, SEED, f)
    shards = [ctx.batch_run_shard(job.inputs[f:f + c], RATE, "lpcm16", job_samples=n, metronome=(g == 0)) for g, (ctx, (f, c)) in enumerate(zip(ctxs, split))]
    got = shards[0][0] + shards[1][0]
    for c in range(NCH):
        assert np.array_equal(got[c], single[c]), "chain output %d" % c
    assert np.array_equal(shards[0][3], single[NCH + 2]), "the metronome track"
    lefts, rights, aux = [s[1] for s in shards], [s[2] for s in shards], shards[0][4]
    # a sharded sum is associated differently from the single context's: the sums as IEEE64, then their restatement
    sums = [b.view(np.float64) for b in ctxs[0].batch_finish_master("ieee64", lefts, rights, aux=aux)]
    want = [ref.encode("lpcm16", sums[0], SEED, ref.PORT_LEFT, 0), ref.encode("lpcm16", sums[1], SEED, ref.PORT_RIGHT, 0)]
    ctxs[0].batch_dither_seek(12345)                                       # the whole-job finish starts at 0 whatever the cursor says
    whole = ctxs[0].batch_finish_master("lpcm16", lefts, rights, aux=aux)
    for side in range(2):
        assert np.array_equal(whole[side], want[side]), "finish_master, side %d" % side
    # ... in two slices (1 + 2 blocks): the cursor walks
    ctxs[0].batch_dither_seek(0)
    cut = lambda a, b: dict(lefts=[p[a:b] for p in lefts], rights=[p[a:b] for p in rights], aux=aux[a:b])
    first = ctxs[0].batch_finish_master_slice("lpcm16", **cut(0, BLOCK))
    second = ctxs[0].batch_finish_master_slice("lpcm16", **cut(BLOCK, n))
    for side in range(2):
        assert np.array_equal(np.concatenate([first[side], second[side]]), want[side]), "two slices, side %d" % side
    # ... and the second slice on a fresh context that seeks to where the first one ended
    fresh = pkg.Context(1, BLOCK)
    fresh.batch_set_dither(1, SEED, 0)
    fresh.batch_dither_seek(BLOCK)
    again = fresh.batch_finish_master_slice("lpcm16", **cut(BLOCK, n))
    for side in range(2):
        assert np.array_equal(again[side], second[side]), "after a seek, side %d" % side
    # a slice that would pass 2^64 is refused
    fresh.batch_dither_seek(2 ** 64 - BLOCK)
    with pytest.raises(pkg.GdgError, match="2\\^64") as e:
        fresh.batch_finish_master_slice("lpcm16", **cut(BLOCK, n))
    assert e.value.code == pkg.GDG_ERR_INVALID
    fresh.close()
    for ctx in ctxs:
        ctx.close()


def test_finish_master_over_several_pieces_and_a_ragged_length():
    """With 2 shards and aux a piece of the finish is 25 blocks: 26 blocks + 5 samples cross a piece boundary (the second piece starts at
    index first + 25 * 8192) and end in a piece whose length is no multiple of 4; the slice form does the same from a cursor below 2^32
    that the job carries across it."""
    pkg = package()
    n, m = 26 * BLOCK + 5, 26 * BLOCK
    rng = np.random.default_rng(41)
    lefts, rights = [rng.uniform(-0.6, 0.6, n) for _ in range(2)], [rng.uniform(-0.6, 0.6, n) for _ in range(2)]
    aux = rng.uniform(-0.3, 0.3, n)
    ctx = pkg.Context(1, BLOCK)
    ctx.batch_set_dither(1, SEED, 0)
    sums = [b.view(np.float64) for b in ctx.batch_finish_master("ieee64", lefts, rights, aux=aux)]
    assert np.array_equal(sums[0], (lefts[0] + lefts[1]) + aux) and np.abs(sums[0]).max() > 1.0
    for fmt in ("lpcm16", "lpcm24"):
        got = ctx.batch_finish_master(fmt, lefts, rights, aux=aux)
        for side, port in enumerate((ref.PORT_LEFT, ref.PORT_RIGHT)):
            want = ref.encode(fmt, sums[side], SEED, port, 0)
            assert got[side].size == want.size and np.array_equal(got[side], want), "%s, side %d: %d bytes differ" % (fmt, side, np.count_nonzero(got[side] != want))
    first = 2 ** 32 - 3 * BLOCK
    ctx.batch_dither_seek(first)
    got = ctx.batch_finish_master_slice("lpcm16", [p[:m] for p in lefts], [p[:m] for p in rights], aux=aux[:m])
    for side, port in enumerate((ref.PORT_LEFT, ref.PORT_RIGHT)):
        assert np.array_equal(got[side], ref.encode("lpcm16", sums[side][:m], SEED, port, first)), "slice, side %d" % side
    # ... and the cursor stands behind the slice
    nxt = ctx.batch_finish_master_slice("lpcm16", [p[:BLOCK] for p in lefts], [p[:BLOCK] for p in rights], aux=aux[:BLOCK])
    assert np.array_equal(nxt[0], ref.encode("lpcm16", sums[0][:BLOCK], SEED, ref.PORT_LEFT, first + m))
    ctx.close()


def test_off_is_off(job):
    rows = job.rows()
    never, never_report, never_kib = job.run("lpcm16", None, report=True)
    ctx = job.configured()
    ctx.batch_set_dither(1, SEED, 0)
    ctx.batch_set_dither(0, SEED, 0xffffffff)                               # off: port_base is not used and cannot be refused
    ctx.batch_report_enable()
    back = ctx.batch_run(job.inputs, RATE, "lpcm16", **KW)
    back_kib = ctx.get_option("stat_batch_device_kib")
    plain = [ctx.wave_encode("lpcm16", r) for r in rows]
    ctx.close()
    for r in range(NCH + 3):
        assert np.array_equal(never[r], plain[r]), "never configured: output %d" % r
        assert np.array_equal(back[r], plain[r]), "mode 1 and back to 0: output %d" % r
    assert never_kib == back_kib and never_kib > 0
    on, on_report, on_kib = job.run("lpcm16", SEED, report=True)
    assert on_report == never_report and len(on_report) == (NCH + 3) * BLOCKS * 32
    assert on_kib == never_kib                                              # the dithered kernels need no memory of their own
    assert np.array_equal(on[0], job.run("lpcm16", SEED)[0][0])
    # IEEE outputs are never dithered
    assert np.array_equal(job.run("ieee64", SEED)[0][NCH], job.run("ieee64", None)[0][NCH])


def test_keys_matter(job):
    """two seeds, one seed twice; and with a source map four equal rows become four different files"""
    a, b = job.run("lpcm16", SEED)[0], job.run("lpcm16", SEED + 1)[0]
    pkg = job.pkg
    ctx = job.configured()
    ctx.batch_set_dither(1, SEED + 2, 0xfffffffd - NCH - 1)                  # the last port_base that fits
    ctx.batch_set_dither(1, SEED, 0)
    # a refused setting leaves the one in force
    for bad in (lambda: ctx.batch_set_dither(2, SEED + 1, 0), lambda: ctx.batch_set_dither(-1, SEED + 1, 0), lambda: ctx.batch_set_dither(1, SEED + 1, 0xfffffffd - NCH)):
        with pytest.raises(pkg.GdgError) as e:
            bad()
        assert e.value.code == pkg.GDG_ERR_INVALID and len(str(e.value)) > len("gdg error -1: ")
    twice = ctx.batch_run(job.inputs, RATE, "lpcm16", **KW)
    ctx.close()
    for r in range(NCH + 3):
        assert np.array_equal(a[r], twice[r]), r
        assert not np.array_equal(a[r], b[r]), r
    outs = {}
    for fmt in ("ieee64", "lpcm16"):
        ctx = job.configured(same_chain=True)
        ctx.batch_set_sources([0, 0, 0, 0])
        ctx.batch_set_dither(1, SEED, 0)
        outs[fmt] = ctx.batch_run([job.inputs[0], None, None, None], RATE, fmt, **KW)
        ctx.close()
    rows = [o.view(np.float64) for o in outs["ieee64"][:NCH]]
    files = [o.view("<i2") for o in outs["lpcm16"][:NCH]]
    for c in range(1, NCH):
        assert np.array_equal(rows[c], rows[0]), c
    for i in range(NCH):
        assert np.array_equal(outs["lpcm16"][i], ref.encode("lpcm16", rows[i], SEED, i, 0)), i
        for j in range(i + 1, NCH):
            frac = np.mean(files[i] != files[j])
            print("files %d and %d differ in %.1f %% of their samples" % (i, j, 100 * frac))
            assert frac > 0.30, (i, j, frac)
