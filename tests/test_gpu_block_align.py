"""The alignment record of the render report (include/gdg.h, gdg_block_align_rows) on the device.

Stand-alone entry: known answers (an impulse against a shifted, scaled impulse; silence; a row against itself; an unmeasured row) and
seeded noise against the numpy restatement (tests/align_ref.py).  The bound is the band spectrum's, the same transforms against the same
kind of restatement: corr and corr0 within 1e-12 * S, S = sqrt(ref_sq * sum_n y[n]^2) of the restatement; ref_sq and sq_at_lag within
1e-12 relative.  Every noise case first asserts, on the restatement alone, that the peak of |r| stands at least 1 % of S above the
runner-up, so that the device's rounding (a few 1e-16 of S) cannot move the argmax; then `lag` is equal.

Largest deviations seen on an MI355X (printed by the tests): corr, corr0: 1.2e-15 * S; ref_sq, sq_at_lag: 2.9e-16 relative.

Batch runs (3 channels x 4 blocks, channel 1 a reader of channel 0's input behind a delaying, inverting power amp, dither on, LPCM24
out): the records equal -- on the bytes -- the stand-alone entry's on the float64 rows of the same job rendered to IEEE64, and do not
depend on the window, the slicing, the sharding or the other two switches of the report."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import align_ref as ref
from helpers import package, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
RATE = 48000
_worst = {"corr": 0.0, "energy": 0.0}


@pytest.fixture(scope="module")
def ctx():
    pkg = package()
    pkg.build()
    c = pkg.Context(1, BLOCK)
    yield c
    c.close()


def check_against_ref(got, rows, refs, M, what, need_margin=True):
    """every measured record against the restatement's: lag equal, corr and corr0 within 1e-12 * S, the energies within 1e-12 relative"""
    for p, q in enumerate(refs):
        for j in range(got.shape[1]):
            g = got[p, j]
            if q < 0:
                assert g.tobytes() == bytes(40), "%s: an unmeasured row's record is all zero" % what
                continue
            want, r, y_sq = ref.record(rows[q][j * BLOCK:(j + 1) * BLOCK], rows[p][j * BLOCK:(j + 1) * BLOCK], M)
            S = np.sqrt(want["ref_sq"] * y_sq)
            if need_margin:
                assert ref.margin(r, M) >= 0.01 * S, "%s: row %d block %d: the case's peak is not distinct enough (a matter of the case, not of the device)" % (what, p, j)
            print("%s row %d block %d: lag %d (want %d) corr %r (want %r) S %r" % (what, p, j, g["lag"], want["lag"], g["corr"], want["corr"], S))
            assert g["lag"] == want["lag"] and g["reserved"] == 0, (what, p, j, int(g["lag"]), want["lag"])
            for f in ("corr", "corr0"):
                if S > 0.0:
                    _worst["corr"] = max(_worst["corr"], abs(g[f] - want[f]) / S)
                assert abs(g[f] - want[f]) <= 1e-12 * S, (what, p, j, f, float(g[f]), want[f], S)
            for f in ("ref_sq", "sq_at_lag"):
                if want[f] > 0.0:
                    _worst["energy"] = max(_worst["energy"], abs(g[f] - want[f]) / want[f])
                assert abs(g[f] - want[f]) <= 1e-12 * want[f], (what, p, j, f, float(g[f]), want[f])
    print("%s: worst so far: corr %.3e * S, energies %.3e relative" % (what, _worst["corr"], _worst["energy"]))


# ---- known answers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 64, 2048])
def test_impulses_give_the_shift_and_the_gain(ctx, M):
    n0 = 4000                                                        # central for every M: M <= n0 < 8192 - M, and n0 + d inside the block
    for a in (0.75, -2.0):
        shifts = sorted({0, 1, -1, M, -M, min(37, M), -min(37, M)})
        rows = np.zeros((1 + len(shifts), BLOCK))
        rows[0, n0] = 1.0
        for i, d in enumerate(shifts):
            rows[1 + i, n0 + d] = a
        got = ctx.block_align(rows, [-1] + [0] * len(shifts), M)
        assert got[0, 0].tobytes() == bytes(40)
        for i, d in enumerate(shifts):
            g = got[1 + i, 0]
            assert g["lag"] == d, "a = %r: a port that arrives %d samples after its reference has lag %d, got %d" % (a, d, d, g["lag"])
            S = abs(a)                                               # sqrt(ref_sq * sum y^2) = sqrt(1 * a^2)
            assert abs(g["corr"] - a) <= 1e-12 * S and abs(g["corr0"] - (a if d == 0 else 0.0)) <= 1e-12 * S, (a, d, g)
            assert abs(g["ref_sq"] - 1.0) <= 1e-12 and abs(g["sq_at_lag"] - a * a) <= 1e-12 * a * a
            assert abs(g["corr"] / np.sqrt(g["ref_sq"] * g["sq_at_lag"]) - np.sign(a)) <= 1e-9
        check_against_ref(got, rows, [-1] + [0] * len(shifts), M, "impulses, M = %d, a = %r" % (M, a))


def test_the_sign_of_the_lag(ctx):
    """+37 against -37: the port that arrives LATER than its reference has the positive lag"""
    rows = np.zeros((3, BLOCK))
    rows[0, 3000], rows[1, 3037], rows[2, 2963] = 1.0, 1.0, 1.0
    got = ctx.block_align(rows, [-1, 0, 0], 64)
    assert (got[1, 0]["lag"], got[2, 0]["lag"]) == (37, -37)
    back = ctx.block_align(rows, [1, -1, -1], 64)                    # ... and the reference measured against the late port arrives earlier
    assert back[0, 0]["lag"] == -37


def test_silence_self_and_unmeasured(ctx):
    rng = np.random.default_rng(21)
    rows = np.zeros((3, 2 * BLOCK))
    rows[2] = rng.uniform(-1.0, 1.0, 2 * BLOCK)
    rows[1, :] = -0.0
    got = ctx.block_align(rows, [1, 0, 2], 64)
    for p in (0, 1):                                                 # two silent blocks: the tie rule decides, zeros everywhere
        for j in range(2):
            assert got[p, j].tobytes() == bytes(40), (p, j, got[p, j])
    for j in range(2):
        g = got[2, j]
        assert g["lag"] == 0 and abs(g["corr"] - g["ref_sq"]) <= 1e-12 * np.sqrt(g["ref_sq"] * float(np.sum(rows[2, j * BLOCK:(j + 1) * BLOCK] ** 2)))
        assert g["corr"] == g["corr0"] and abs(g["sq_at_lag"] - g["ref_sq"]) <= 1e-12 * g["ref_sq"]       # the same samples, summed in two orders
    none = ctx.block_align(rows, [-1, -1, -1], 64)
    assert none.tobytes() == bytes(40 * 6)
    check_against_ref(got, rows, [1, 0, 2], 64, "silence and self", need_margin=False)


# ---- against the restatement -------------------------------------------------------------------------------------------------------
def noise_rows(seed, samples, g, d):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(samples)
    y = np.zeros(samples)
    if d >= 0:
        y[d:] = x[:samples - d]
    else:
        y[:samples + d] = x[-d:]
    return x, g * y, rng


@pytest.mark.parametrize("n_rows,samples,M,g,d", [
    (2, 8192, 2048, 0.5, 37), (2, 8192, 2048, -1.5, -2048), (3, 8193, 64, -0.5, 64), (3, 2 * 8192, 64, 1.5, -5), (1, 100, 1, 1.0, 0),
    (2, 100, 1, -1.0, 1), (2, 8192, 1, 0.5, -1), (3, 8193, 2048, 1.5, 2048), (2, 2 * 8192, 2048, -0.5, 700), (2, 100, 64, 1.5, -9)])
def test_noise_against_the_restatement(ctx, n_rows, samples, M, g, d):
    x, y, rng = noise_rows(100 + abs(d) + M, samples, g, d)
    clean = [x, y, y + 0.01 * rng.standard_normal(samples)][:max(n_rows, 1)] if n_rows > 1 else [x]
    refs = [0, 0, 0][:len(clean)]
    got = ctx.block_align(np.stack(clean), refs, M)
    assert got.shape == (len(clean), -(-samples // BLOCK))
    check_against_ref(got, clean, refs, M, "noise %d x %d, M = %d, g = %r, d = %d" % (n_rows, samples, M, g, d))
    if n_rows > 1:                                                   # the noise-free pair: the coefficient is +-1 where the shifted copy covers the slice
        for j in range(got.shape[1]):
            lo, hi = j * BLOCK, min((j + 1) * BLOCK, samples)
            covered = (M + d >= 0 if j == 0 else True) and (BLOCK - M + d <= hi - lo)
            rec = got[1, j]
            if covered and rec["ref_sq"] > 0.0:
                assert abs(rec["corr"] / np.sqrt(rec["ref_sq"] * rec["sq_at_lag"]) - np.sign(g)) <= 1e-9, (j, rec)


def device_records(ctx, stored, offset, stride, n_rows, samples, refs, M):
    """gdg_block_align_rows_device on rows `stride` samples apart from sample `offset` of the flat array `stored`"""
    pkg = package()
    n = n_rows * -(-samples // BLOCK) * 5
    d_in, d_out = pkg.DeviceBuffer(ctx, 1, stored.size), pkg.DeviceBuffer(ctx, 1, n + 4)
    try:
        d_in.upload(stored)
        d_out.upload(np.full(n + 4, -7.0))
        ctx.block_align_device(d_in.ptr + 8 * offset, stride, n_rows, samples, refs, M, d_out.ptr)
        ctx.synchronize()
        raw = d_out.download().reshape(-1)
        assert np.all(raw[n:] == -7.0), "a record was written past the last one"
        return raw[:n].copy().view(ref.DTYPE).reshape(n_rows, -1)
    finally:
        d_in.free()
        d_out.free()


def test_nothing_outside_the_row_is_read_and_alignment_changes_no_bit(ctx):
    samples, M = BLOCK + 100, 64
    x, y, _ = noise_rows(5, samples, -0.5, 9)
    host = ctx.block_align(np.stack([x, y]), [0, 0], M)
    refs = [0, 0, -1]
    for offset, stride in ((4, samples + 4), (5, samples + 4), (0, samples + 1)):      # pair loads; 8 bytes off; an odd stride: row 1 8 bytes off
        stored = np.full(offset + 3 * stride + 8192 + 11, np.nan)
        for r, row in enumerate((x, y, x)):
            stored[offset + r * stride:offset + r * stride + samples] = row
        dev = device_records(ctx, stored, offset, stride, 3, samples, refs, M)
        assert np.all(np.isfinite(dev["corr"])) and np.all(np.isfinite(dev["sq_at_lag"])), "offset %d: a sample outside the row was read" % offset
        assert dev[:2].tobytes() == host.tobytes(), "offset %d stride %d" % (offset, stride)
        assert dev[2].tobytes() == bytes(80), "the unmeasured row's records are zeroed"


def test_non_finite_samples_count_as_zero(ctx):
    x, y, _ = noise_rows(6, BLOCK, 1.5, -20)
    xz, yz = x.copy(), y.copy()
    xn, yn = x.copy(), y.copy()
    xz[[77, 4097]] = 0.0
    yz[[5, 8000]] = 0.0
    xn[77], xn[4097], yn[5], yn[8000] = np.nan, np.inf, -np.inf, np.nan
    a, b = ctx.block_align(np.stack([xz, yz]), [1, 0], 64), ctx.block_align(np.stack([xn, yn]), [1, 0], 64)
    assert a.tobytes() == b.tobytes() and np.all(np.isfinite(b["corr"])) and b[1, 0]["lag"] == -20 and b[0, 0]["lag"] == 20


def test_refusals_of_the_stand_alone_entry(ctx):
    pkg = package()
    lib = pkg.lib()
    r2 = np.array([0, 0], dtype=np.int32)
    bad = np.array([0, 2], dtype=np.int32)
    for rc in (lib.gdg_block_align_rows_device(ctx._h, 8, 4, 2, 8, r2.ctypes.data, 64, 8),               # stride < samples
               lib.gdg_block_align_rows_device(ctx._h, 12, 8, 2, 8, r2.ctypes.data, 64, 8),              # a 4-byte aligned row
               lib.gdg_block_align_rows_device(ctx._h, 8, 8, 2, 8, r2.ctypes.data, 0, 8),                # no lag range
               lib.gdg_block_align_rows_device(ctx._h, 8, 8, 2, 8, r2.ctypes.data, 2049, 8),
               lib.gdg_block_align_rows_device(ctx._h, 8, 8, 2, 8, bad.ctypes.data, 64, 8),              # a reference past the list
               lib.gdg_block_align_rows_device(ctx._h, 8, 8, 2, 8, None, 64, 8)):
        assert rc == pkg.GDG_ERR_INVALID and lib.gdg_last_error(ctx._h)
    assert ctx.block_align(np.zeros((2, 16)), [0, 0], 1).shape == (2, 1)     # the context stays usable


# ---- batch runs --------------------------------------------------------------------------------------------------------------------
NCH, BLOCKS, M_JOB = 3, 4, 64
KW = dict(metronome_to_master=True)
FIR = np.array([0.0, 0.0, 0.0, 0.0, 0.0, -0.9, 0.1])                 # channel 1: five samples late, inverted
POSITIONS = [(-35.0, 0.6, 1.0), (40.0, 0.8, 0.9), (5.0, 0.7, 0.8)]
SOURCES = [0, 0, 2]                                                  # channel 1 reads channel 0's input
REFS = [0, 0, 0, 0, 3, 5]                                            # the chains against channel 0, master left against it, right against left, the metronome itself
_job = {}


def the_job():
    if "job" in _job:
        return _job["job"]
    pkg = package()
    n = BLOCKS * BLOCK
    x0 = 0.4 * synth_signal(0, n, RATE)
    x2 = 0.5 * synth_signal(7, 30000, 44100)                         # resampled; covers 32654 of the job's 32768 samples
    tick, tock = 0.008 * np.sin(np.arange(600) * 0.2), 0.006 * np.sin(np.arange(400) * 0.3)
    enc = lambda x: np.frombuffer(np.asarray(x, dtype="<f8").tobytes(), dtype=np.uint8)
    inputs = [(enc(x0), "ieee64", RATE), None, (enc(x2), "ieee64", 44100)]

    def configured(first=0, count=NCH, refs=REFS, report=False, edges=None, dither=True):
        ctx = pkg.Context(count, BLOCK)
        if first <= 1 < first + count:
            ctx.append_unit(1 - first, "power_amp", fir=FIR)
        if first <= 2 < first + count:
            ctx.append_unit(2 - first, "overdrive", params=[0, 15, 80, -3, 1, 0])
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(count):
            ctx.spatializer_set_position(c, *POSITIONS[first + c])
        ctx.metronome_set_sounds(tick, tock)
        ctx.metronome_configure(3, 200, RATE)
        ctx.set_window(2)
        ctx.batch_set_sources([s - first for s in SOURCES[first:first + count]])
        if dither:
            ctx.batch_set_dither(1, seed=99, port_base=first)
        if refs is not None:
            ctx.batch_align_enable(refs, M_JOB)
        if report:
            ctx.batch_report_enable()
        if edges is not None:
            ctx.batch_spectrum_enable(edges)
        return ctx

    _job["job"] = SimpleNamespace(inputs=inputs, configured=configured, length=n)
    return _job["job"]


def one_call(job, fmt="lpcm24", W=2, **cfg):
    ctx = job.configured(**cfg)
    ctx.set_window(W)
    res = ctx.batch_run(job.inputs, RATE, fmt, **KW)
    rec = ctx.batch_align()
    ctx.close()
    return [o.tobytes() for o in res], rec


@pytest.fixture(scope="module")
def plain():
    package().build()
    job = the_job()
    raw, rec = one_call(job)
    return job, raw, rec


def slice_inputs(datas, widths, need):
    return [None if d is None or not c else d[f * w:(f + c) * w] for d, w, (f, c) in zip(datas, widths, need)]


def streamed(job, slicing, W, **cfg):
    ctx = job.configured(**cfg)
    ctx.set_window(W)
    metas, datas, widths = ctx._stream_split(job.inputs)
    ctx.batch_stream_open(metas, RATE, "lpcm24", **KW)
    parts, recs = [], []
    for k in slicing:
        parts.append(ctx.batch_stream_step(k, slice_inputs(datas, widths, ctx.batch_stream_need(k))))
        recs.append(ctx.batch_align())
        assert recs[-1].shape == (NCH + 3, k)
    ctx.batch_stream_close()
    ctx.close()
    return [b"".join(p[r].tobytes() for p in parts) for r in range(NCH + 3)], np.concatenate(recs, axis=1)


def test_batch_equals_the_stand_alone_entry_on_the_float64_rows(plain, ctx):
    job, raw, rec = plain
    assert rec.shape == (NCH + 3, BLOCKS) and rec.dtype.itemsize == 40
    raw64, rec64 = one_call(job, "ieee64")
    rows = np.stack([np.frombuffer(b, dtype="<f8") for b in raw64])
    alone = ctx.block_align(rows, REFS, M_JOB)
    assert rec.tobytes() == alone.tobytes(), "LPCM24 job, dither on: the records of the float64 rows, in the order of out_bytes"
    assert rec64.tobytes() == alone.tobytes()
    check_against_ref(rec, rows, REFS, M_JOB, "batch run", need_margin=False)
    assert np.all(rec[1]["lag"] == 5) and np.all(rec[1]["corr"] < 0.0), "channel 1: five samples behind channel 0, inverted"
    assert np.all(rec[0]["lag"] == 0) and np.all(rec[5]["lag"] == 0)


def test_records_do_not_depend_on_window_or_slicing(plain):
    job, raw, rec = plain
    for W in (1, 2):
        raw_w, rec_w = one_call(job, W=W)
        assert rec_w.tobytes() == rec.tobytes() and raw_w == raw, "one call, window %d" % W
        for slicing in ((1, 1, 1, 1), (3, 1)):
            raw_s, rec_s = streamed(job, slicing, W)
            assert rec_s.tobytes() == rec.tobytes() and raw_s == raw, "slices %r, window %d" % (slicing, W)


def test_records_of_a_sharded_job(plain):
    """channels 0 and 1 (a root and its reader) on one shard context, channel 2 on another: chain and metronome ports on the bytes"""
    job, raw, rec = plain
    slicing = (1, 3)
    # shard 0: ports ch0, ch1, metronome; shard 1: ports ch2, metronome (not run there): a reference on another shard cannot be measured
    ctxs = [job.configured(0, 2, refs=[0, 0, 2]), job.configured(2, 1, refs=[0, 1])]
    gens = []
    for g, (c, (f, n)) in enumerate(zip(ctxs, ((0, 2), (2, 1)))):
        it = iter(slicing)
        gens.append(c.batch_stream_shard(job.inputs[f:f + n], RATE, "lpcm24", lambda left, it=it: next(it), job_samples=job.length, metronome=(g == 0)))
    own2 = None
    at = 0
    for k in slicing:
        parts = [next(gen) for gen in gens]
        recs = [c.batch_align() for c in ctxs]
        assert recs[0].shape == (3, k) and recs[1].shape == (2, k)
        here = rec[:, at:at + k]
        assert recs[0][0].tobytes() == here[0].tobytes() and recs[0][1].tobytes() == here[1].tobytes(), "chain outputs of shard 0"
        assert recs[0][2].tobytes() == here[NCH + 2].tobytes(), "the metronome, from the shard that runs it"
        assert recs[1][1].tobytes() == bytes(40 * k), "all-zero on the shard that does not"
        own2 = recs[1][0] if own2 is None else np.concatenate([own2, recs[1][0]])
        ctxs[1].batch_finish_master_slice("lpcm24", [p[1] for p in parts], [p[2] for p in parts], aux=parts[0][4], sample_rate=RATE)
        with pytest.raises(package().GdgError, match="no alignment records"):
            ctxs[1].batch_align()                                    # the finish carries none
        at += k
    for gen in gens:
        assert next(gen, None) is None
    for c in ctxs:
        c.close()
    # channel 2 against itself, as the single context measures it with such a list
    _, self2 = one_call(job, refs=[0, 0, 2, -1, -1, 5])
    assert own2.tobytes() == self2[2].tobytes() and self2[:2].tobytes() == rec[:2].tobytes() and self2[5].tobytes() == rec[5].tobytes()
    assert self2[3:5].tobytes() == bytes(40 * 2 * BLOCKS)


def test_switches(plain):
    pkg = package()
    job, raw, rec = plain
    edges = [100.0, 1000.0, 10000.0]
    run = lambda c: [o.tobytes() for o in c.batch_run(job.inputs, RATE, "lpcm24", **KW)]
    never = job.configured(refs=None, report=True, edges=edges)
    assert run(never) == raw, "alignment on changes no output byte"
    rep, bands, kib = never.batch_report(), never.batch_spectrum(), never.get_option("stat_batch_device_kib")
    with pytest.raises(pkg.GdgError) as e:
        never.batch_align()
    assert e.value.code == pkg.GDG_ERR_INVALID and "no alignment records" in str(e.value)        # before any call with it
    never.close()
    off = job.configured(report=True, edges=edges)
    off.batch_align_enable(None)
    assert run(off) == raw
    assert off.batch_report().tobytes() == rep.tobytes() and off.batch_spectrum().tobytes() == bands.tobytes() and off.get_option("stat_batch_device_kib") == kib
    with pytest.raises(pkg.GdgError):
        off.batch_align()
    off.close()
    # all three on: each of them what it is alone (`plain` is alignment alone)
    three = job.configured(report=True, edges=edges)
    assert run(three) == raw
    assert three.batch_align().tobytes() == rec.tobytes() and three.batch_report().tobytes() == rep.tobytes() and three.batch_spectrum().tobytes() == bands.tobytes()
    three.close()
    for cfg in (dict(report=True), dict(edges=edges)):
        raw_s, rec_s = streamed(job, (2, 2), 2, **cfg)
        assert raw_s == raw and rec_s.tobytes() == rec.tobytes()
    # dither off: other bytes, the same records (they are taken in front of it)
    raw_d, rec_d = one_call(job, dither=False)
    assert rec_d.tobytes() == rec.tobytes() and raw_d != raw


def test_refusals(plain):
    pkg = package()
    job, raw, rec = plain
    lib = pkg.lib()
    c = job.configured(refs=None)
    with pytest.raises(pkg.GdgError, match="no alignment records"):
        c.batch_align()                                              # before any call
    # a list of the wrong length for the call: refused before anything is done, and the context stays usable
    c.batch_align_enable([0, 0, 0, 0], M_JOB)                        # a shard's count
    with pytest.raises(pkg.GdgError) as e:
        c.batch_run(job.inputs, RATE, "lpcm24", **KW)
    assert e.value.code == pkg.GDG_ERR_INVALID and "4 ports, this call 6" in str(e.value)
    # a refused list leaves the one in force
    bad = np.array([0, 6, 0, 0, 0, 0], dtype=np.int32)
    assert lib.gdg_batch_align_enable(c._h, bad.ctypes.data, 6, M_JOB) == pkg.GDG_ERR_INVALID and b"port 1" in lib.gdg_last_error(c._h)
    good = np.array(REFS, dtype=np.int32)
    assert lib.gdg_batch_align_enable(c._h, good.ctypes.data, 6, 0) == pkg.GDG_ERR_INVALID
    assert lib.gdg_batch_align_enable(c._h, good.ctypes.data, 6, 2049) == pkg.GDG_ERR_INVALID
    with pytest.raises(pkg.GdgError):
        c.batch_run(job.inputs, RATE, "lpcm24", **KW)                # still the list of four
    c.batch_align_enable(REFS, M_JOB)
    # while a streamed job is open the switch is refused and nothing changes
    metas, datas, widths = c._stream_split(job.inputs)
    c.batch_stream_open(metas, RATE, "lpcm24", **KW)
    assert lib.gdg_batch_align_enable(c._h, good.ctypes.data, 6, 1) == pkg.GDG_ERR_INVALID and b"streamed batch run is open" in lib.gdg_last_error(c._h)
    assert lib.gdg_batch_align_enable(c._h, None, 0, 0) == pkg.GDG_ERR_INVALID
    outs = c.batch_stream_step(BLOCKS, slice_inputs(datas, widths, c.batch_stream_need(BLOCKS)))
    assert c.batch_align().tobytes() == rec.tobytes() and [o.tobytes() for o in outs] == raw
    c.batch_stream_close()
    # too little room says so, with the counts
    ports, blocks = C.c_int(0), C.c_size_t(0)
    few = np.zeros(5, dtype=pkg.BLOCK_ALIGN_DTYPE)
    assert lib.gdg_batch_align(c._h, few.ctypes.data, few.size, C.byref(ports), C.byref(blocks)) == pkg.GDG_ERR_INVALID
    assert (ports.value, blocks.value) == (NCH + 3, BLOCKS) and b"room for 5 records" in lib.gdg_last_error(c._h)
    c.close()
