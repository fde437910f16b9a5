"""The render report (include/gdg.h, gdg_block_stats): peak, sum of squares and three counts per block of every row.

Stand-alone entry (gdg_block_stats_rows / _rows_device): against numpy -- peak, peak_index and the three counts exactly; sum_sq against
math.fsum of the squares of the finite samples within n * 2^-52 relative for a block of n samples (n roundings of squares and n - 1
additions of non-negative terms give at most about n * 2^-53 in ANY order; the bound allows a factor two over that) -- and, for the same
8192 samples placed in different rows, blocks and alignments, bit-identical.

Batch runs (3 channels, 5 blocks, IEEE64 out, meters off): the decoded IEEE64 bytes ARE the pre-encode samples, so the records of every
block that holds no clipped and no non-finite sample are checked against numpy on the decoded file; the records of the one-call run, of
streamed slices, of two windows, of a resumed job and of a sharded job are byte-equal where the output files are."""
import math

import numpy as np
import pytest

from helpers import package, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
EPS = 2.0 ** -52


# ---- numpy's side ------------------------------------------------------------------------------------------------------------------
def ref_stats(x, block):
    """the records of one row as include/gdg.h defines them; sum_sq = math.fsum of the (rounded) squares"""
    pkg = package()
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(-(-x.size // block), dtype=pkg.BLOCK_STATS_DTYPE)
    for b in range(out.size):
        seg = x[b * block:(b + 1) * block]
        fin = np.isfinite(seg)
        a = np.abs(seg[fin])
        at = np.nonzero(fin)[0]
        peak = float(a.max()) if a.size else 0.0
        out[b] = (peak, math.fsum(float(v) * float(v) for v in seg[fin]), int(at[int(np.argmax(a))]) if peak > 0.0 else 0,
                  int((a > 1.0).sum()), int((a >= 1.0).sum()), int((~fin).sum()))
    return out


def check_records(got, want, lengths, what):
    """exact fields exactly, sum_sq within n * 2^-52 relative (n = the block's samples)"""
    assert got.shape == want.shape, what
    for name in ("peak", "peak_index", "clipped", "full_scale", "nonfinite"):
        assert np.array_equal(got[name], want[name]), "%s: %s\n got %s\nwant %s" % (what, name, got[name], want[name])
    for i, (g, w, n) in enumerate(zip(got["sum_sq"].ravel(), want["sum_sq"].ravel(), np.broadcast_to(lengths, got.shape).ravel())):
        assert abs(g - w) <= n * EPS * w, "%s: sum_sq of record %d: %r against %r (%d samples)" % (what, i, g, w, n)


def block_lengths(samples, block):
    return np.array([min(block, samples - b * block) for b in range(-(-samples // block))])


def device_records(ctx, stored, offset, stride, n_rows, samples, block):
    """gdg_block_stats_rows_device on rows that lie `stride` samples apart from sample `offset` of the flat array `stored`"""
    pkg = package()
    nblk = -(-samples // block)
    d_in = pkg.DeviceBuffer(ctx, 1, stored.size)
    d_rec = pkg.DeviceBuffer(ctx, 1, 4 * n_rows * nblk + 4)
    try:
        d_in.upload(stored)
        d_rec.upload(np.full(4 * n_rows * nblk + 4, -7.0))
        ctx.block_stats_device(d_in.ptr + 8 * offset, stride, n_rows, samples, block, d_rec.ptr)
        ctx.synchronize()
        raw = d_rec.download().reshape(-1)
        assert np.all(raw[4 * n_rows * nblk:] == -7.0), "a record was written past the last one"
        return raw[:4 * n_rows * nblk].copy().view(pkg.BLOCK_STATS_DTYPE).reshape(n_rows, nblk)
    finally:
        d_in.free()
        d_rec.free()


@pytest.fixture(scope="module")
def ctx():
    pkg = package()
    pkg.build()
    c = pkg.Context(1, BLOCK)
    yield c
    c.close()


def test_symbols_exist():
    pkg = package()
    assert all(hasattr(pkg.lib(), n) for n in ("gdg_block_stats_rows", "gdg_block_stats_rows_device", "gdg_batch_report_enable", "gdg_batch_report"))


# ---- the stand-alone entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [1, 4, 63, 64, 65, 256, 1000, 8192])
@pytest.mark.parametrize("n_rows", [1, 3])
def test_rows_against_numpy(ctx, n_rows, block):
    """host form (compact rows: every other row of an odd length lies 8 bytes past a 16-byte boundary) and device form with a row stride
    larger than the row, the gap filled with NaN and 1e300 -- an over-read shows up in `nonfinite` or `peak` --, a short last block"""
    samples = 3 if block == 1 else 2 * block + block // 2 + 1
    rng = np.random.default_rng(1000 * n_rows + block)
    x = rng.uniform(-1.2, 1.2, (n_rows, samples))
    x[:, ::7] *= 0.01
    want = np.stack([ref_stats(r, block) for r in x])
    lengths = block_lengths(samples, block)
    assert block == 1 or lengths[-1] < block
    got = ctx.block_stats(x, block)
    check_records(got, want, lengths, "host form")
    even = samples + 6 + samples % 2
    for stride, offset in ((even, 0), (even + 1, 2), (even, 1)):    # 16-byte aligned rows (pair loads when the block is even); odd stride;
        # 8 bytes past a 16-byte boundary
        stored = np.empty(offset + n_rows * stride + 8)
        stored[0::2], stored[1::2] = np.nan, 1e300
        for r in range(n_rows):
            stored[offset + r * stride:offset + r * stride + samples] = x[r]
        dev = device_records(ctx, stored, offset, stride, n_rows, samples, block)
        check_records(dev, want, lengths, "device form, stride %d, offset %d" % (stride, offset))
        assert np.array_equal(dev["sum_sq"].view(np.uint64), got["sum_sq"].view(np.uint64)), "sum_sq depends on where the rows lie"


@pytest.mark.parametrize("block", [65, 256])
def test_planted_values(ctx, block):
    tiny, above = 5e-324, np.nextafter(1.0, 2.0)
    rng = np.random.default_rng(block)
    x = rng.uniform(-0.5, 0.5, 8 * block)
    blk = lambda b: x[b * block:(b + 1) * block]
    blk(0)[10] = blk(0)[40] = 0.75                                  # two equal maxima: the lower index wins
    blk(0)[55] = -0.75                                              # ... whatever the sign
    blk(1)[33] = -0.9                                               # a negative peak
    blk(2)[5], blk(2)[6], blk(2)[60] = 1.0, -1.0, above             # full scale is not clipped; one ulp above is
    blk(3)[:] = 0.0
    blk(3)[1], blk(3)[2], blk(3)[3], blk(3)[4], blk(3)[50] = np.nan, np.inf, -np.inf, -0.0, tiny      # the peak is the denormal
    blk(4)[:] = 0.0                                                 # all zero
    blk(5)[0::3], blk(5)[1::3], blk(5)[2::3] = np.nan, np.inf, -np.inf      # nothing finite
    blk(6)[:] = -0.0
    blk(7)[block - 1] = -3.5                                        # the last sample of the last block
    want = ref_stats(x, block)
    assert (want["peak_index"][0], want["peak"][0]) == (10, 0.75) and (want["peak"][1], want["peak_index"][1]) == (0.9, 33)
    assert (want["full_scale"][2], want["clipped"][2], want["peak"][2], want["peak_index"][2]) == (3, 1, above, 60)
    assert (want["nonfinite"][3], want["peak"][3], want["peak_index"][3], want["sum_sq"][3]) == (3, tiny, 50, 0.0)
    assert tuple(want[4]) == (0.0, 0.0, 0, 0, 0, 0) and tuple(want[5]) == (0.0, 0.0, 0, 0, 0, block) and tuple(want[6]) == (0.0, 0.0, 0, 0, 0, 0)
    assert (want["peak"][7], want["peak_index"][7], want["clipped"][7]) == (3.5, block - 1, 1)
    for n_rows in (1, 3):
        rows = [x] + [rng.uniform(-1, 1, x.size) for _ in range(n_rows - 1)]
        got = ctx.block_stats(rows[::-1], block)                    # the planted row is the last one
        check_records(got[-1:], want[None, :], block, "planted values, %d rows" % n_rows)


def test_the_same_samples_give_the_same_bits_wherever_they_sit(ctx):
    rng = np.random.default_rng(5)
    s = rng.uniform(-1.1, 1.1, BLOCK) * rng.uniform(0, 1, BLOCK) ** 3
    other = lambda n: rng.uniform(-1.1, 1.1, n)
    want = ref_stats(s, BLOCK)
    alone = ctx.block_stats(s[None, :], BLOCK)
    check_records(alone, want[None, :], BLOCK, "row 0 of 1")
    bits = alone["sum_sq"].view(np.uint64)[0, 0]
    three = ctx.block_stats([other(BLOCK), other(BLOCK), s], BLOCK)
    long_row = np.concatenate([s, other(BLOCK), s, other(100)])
    longer = ctx.block_stats([other(long_row.size), long_row], BLOCK)
    stored = np.concatenate([other(1), s, other(3)])                # 8 bytes past a 16-byte boundary: single loads, the same order
    shifted = device_records(ctx, stored, 1, BLOCK + 2, 1, BLOCK, BLOCK)
    placed = {"row 2 of 3": three[2, 0], "block 0 of a longer row": longer[1, 0], "block 2 of a longer row": longer[1, 2], "8-byte aligned": shifted[0, 0]}
    for what, rec in placed.items():
        assert rec["sum_sq"].view(np.uint64) == bits, what
        assert rec.tobytes() == alone[0, 0].tobytes(), what
    assert longer[1, 3]["sum_sq"] != alone[0, 0]["sum_sq"] and longer.shape == (2, 4)


def test_refusals(ctx):
    pkg = package()
    for call in (lambda: ctx.block_stats_device(8, 4, 1, 8, 2, 8), lambda: ctx.block_stats_device(12, 8, 1, 8, 2, 8),
                 lambda: pkg.Context._check(ctx, pkg.lib().gdg_block_stats_rows(ctx._h, None, 1, 8, 0, None))):
        with pytest.raises(pkg.GdgError) as e:
            call()
        assert e.value.code == pkg.GDG_ERR_INVALID
    assert ctx.block_stats(np.zeros((2, 0)), 4).shape == (2, 0)


# ---- batch runs --------------------------------------------------------------------------------------------------------------------
RATE, NCH, BLOCKS = 48000, 3, 5
KW = dict(metronome_to_master=True)
FIR = np.array([1.5, 0.45, -0.25, 0.1])                             # a short filter with gain: the amp's clamp leaves exact +-1
POSITIONS = [(-35.0, 0.6, 1.0), (40.0, 0.8, 0.9), (0.0, 1.0, 1.0)]
_job = {}


def report_job(oracle):
    """Channel 0: an empty chain, quiet except inside block 2; channel 1: overdrive -> power amp, driven hard; channel 2 left empty; a
    quiet metronome in the master.  Levels fixed on the CPU oracle: the master exceeds 1 in block 2 only, no chain output ever does."""
    if "job" in _job:
        return _job["job"]
    pkg = package()
    n = BLOCKS * BLOCK
    env = np.full(n, 0.12)
    env[2 * BLOCK + 1000:3 * BLOCK - 1000] = 0.93
    x0 = env * synth_signal(0, n, RATE) / 0.8
    x1 = 0.9 * synth_signal(7, n, RATE)
    tick, tock = 0.008 * np.sin(np.arange(600) * 0.2), 0.006 * np.sin(np.arange(400) * 0.3)
    inputs = [(oracle.wave_encode("ieee64", x0), "ieee64", RATE), (oracle.wave_encode("ieee64", x1), "ieee64", RATE), None]
    # the oracle's rendering: what the levels were fixed on
    ch = oracle.Chain()
    ch.append_unit("overdrive", params=[0, 15, 80, -3, 1, 0])
    ch.append_unit("power_amp", fir=FIR)
    y1 = np.concatenate([ch.process(x1[b * BLOCK:(b + 1) * BLOCK], RATE) for b in range(BLOCKS)])
    sp = oracle.Spatializer(NCH)
    sp.set_sample_rate(RATE)
    for c, (a, d, l) in enumerate(POSITIONS):
        sp.set_azimuth(c, a); sp.set_distance(c, d); sp.set_level(c, l)
    met = oracle.Metronome()
    met.tick, met.tock = tick, tock
    met.s.beats_per_period, met.s.bpm_speed, met.s.sample_rate = 3, 200, RATE
    chain_out = np.stack([x0, y1, np.zeros(n)])
    master = np.zeros((2, n))
    for b in range(BLOCKS):
        sl = slice(b * BLOCK, (b + 1) * BLOCK)
        master[0, sl], master[1, sl] = sp.process(chain_out[:, sl], aux=met.process(BLOCK))
    assert np.abs(chain_out).max() <= 1.0 and (np.abs(y1) == 1.0).sum() > 100, "no chain output exceeds 1; the amp's clamp leaves exact +-1"
    over = [[int((np.abs(m[b * BLOCK:(b + 1) * BLOCK]) > 1.0).sum()) for b in range(BLOCKS)] for m in master]
    assert all(o[2] > 0 for o in over) and all(o[b] == 0 for o in over for b in (0, 1, 3, 4)), over

    def configured(first=0, count=NCH):
        ctx = pkg.Context(count, BLOCK)
        if first <= 1 < first + count:
            ctx.append_unit(1 - first, "overdrive", params=[0, 15, 80, -3, 1, 0])
            ctx.append_unit(1 - first, "power_amp", fir=FIR)
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(count):
            ctx.spatializer_set_position(c, *POSITIONS[first + c])
        ctx.metronome_set_sounds(tick, tock)
        ctx.metronome_configure(3, 200, RATE)
        return ctx

    from types import SimpleNamespace
    _job["job"] = SimpleNamespace(inputs=inputs, configured=configured, length=n)
    return _job["job"]


def one_call(job, W=4, report=True):
    """the one-call run on a fresh context: (decoded float64 outputs [N + 3][n], output bytes, report or None)"""
    ctx = job.configured()
    ctx.set_window(W)
    if report:
        ctx.batch_report_enable()
    outs = ctx.batch_run(job.inputs, RATE, "ieee64", **KW)
    rep = ctx.batch_report() if report else None
    ctx.close()
    return np.stack([o.view(np.float64) for o in outs]), [o.tobytes() for o in outs], rep


@pytest.fixture(scope="module")
def plain(oracle):
    job = report_job(oracle)
    dec, raw, rep = one_call(job)
    return job, dec, raw, rep


def streamed(job, slicing, W=4, skip=()):
    ctx = job.configured()
    ctx.set_window(W)
    ctx.batch_report_enable()
    metas, datas, widths = ctx._stream_split(job.inputs)
    ctx.batch_stream_open(metas, RATE, "ieee64", **KW)
    parts, reps = [], []
    for k in slicing:
        need = ctx.batch_stream_need(k)
        ins = [None if d is None or not c else d[f * w:(f + c) * w] for d, w, (f, c) in zip(datas, widths, need)]
        outs = [None if r in skip else np.zeros(k * BLOCK * 8, dtype=np.uint8) for r in range(NCH + 3)]
        parts.append(ctx.batch_stream_step(k, ins, outs=outs))
        reps.append(ctx.batch_report())
        assert reps[-1].shape == (NCH + 3, k)
    ctx.batch_stream_close()
    ctx.close()
    return parts, np.concatenate(reps, axis=1)


def test_report_against_the_decoded_files(plain):
    job, dec, raw, rep = plain
    assert rep.shape == (NCH + 3, BLOCKS) and dec.shape == (NCH + 3, job.length)
    want = np.stack([ref_stats(r, BLOCK) for r in dec])
    clean = (rep["clipped"] == 0) & (rep["nonfinite"] == 0)
    print("clipped per port-block:\n%s\nfull_scale:\n%s" % (rep["clipped"], rep["full_scale"]))
    assert clean.sum() * 4 >= 3 * clean.size, "at least three quarters of all port-blocks hold no clipped sample: %d of %d" % (clean.sum(), clean.size)
    assert np.array_equal(rep["nonfinite"], np.zeros_like(rep["nonfinite"]))
    for name in ("peak", "peak_index", "full_scale"):
        assert np.array_equal(rep[name][clean], want[name][clean]), name
    for g, w in zip(rep["sum_sq"][clean], want["sum_sq"][clean]):
        assert abs(g - w) <= BLOCK * EPS * w, (g, w)
    # Every block: full_scale against the decoded file.  An encoder that clamps turns every |x| >= 1 into exactly +-1; IEEE64 writes the
    # sample's bytes unclamped (wave.go:694-709), so in its files those samples are the ones with |x| >= 1, and the ones with |x| == 1
    # are full_scale less clipped -- which is full_scale itself wherever nothing is clipped.
    blocks_of = lambda r: [np.abs(r[b * BLOCK:(b + 1) * BLOCK]) for b in range(BLOCKS)]
    assert np.array_equal(rep["full_scale"], np.stack([[(a >= 1.0).sum() for a in blocks_of(r)] for r in dec]))
    assert np.array_equal(rep["full_scale"] - rep["clipped"], np.stack([[(a == 1.0).sum() for a in blocks_of(r)] for r in dec]))
    check_records(rep, want, BLOCK, "every block (IEEE64 keeps what lies above 1, so the clipped blocks can be checked as well)")
    assert rep["clipped"][NCH:NCH + 2].max() > 0, "at least one master block is clipped"
    assert rep["clipped"][:NCH].max() == 0 and rep["clipped"][NCH + 2].max() == 0, "no chain output and no metronome block is"
    assert rep["full_scale"][1].min() > 0, "the power amp's clamp leaves exact +-1 in every block of channel 1"
    assert tuple(rep[2, 0]) == (0.0, 0.0, 0, 0, 0, 0) and rep["peak"][NCH + 2].max() > 0.0          # the empty channel; the metronome


def test_records_do_not_depend_on_slicing_or_window(plain):
    job, dec, raw, rep = plain
    for W in (1, 4):
        for slicing, skip in (((1, 2, 2), ()), ((5,), ()), ((2, 3), (0, NCH))):
            parts, got = streamed(job, slicing, W, skip)
            assert got.tobytes() == rep.tobytes(), "slices %s, window %d, outputs skipped %s" % (slicing, W, skip)
            for r in range(NCH + 3):
                if r not in skip:
                    assert b"".join(p[r].tobytes() for p in parts) == raw[r], "output %d" % r
        assert one_call(job, W)[2].tobytes() == rep.tobytes(), "one-call run, window %d" % W


def test_report_off_is_the_default_and_changes_nothing(plain):
    pkg = package()
    job, dec, raw, rep = plain
    never = job.configured()
    never.set_window(4)
    outs = never.batch_run(job.inputs, RATE, "ieee64", **KW)
    assert [o.tobytes() for o in outs] == raw, "the report on changes no output byte"
    with pytest.raises(pkg.GdgError) as e:
        never.batch_report()
    assert e.value.code == pkg.GDG_ERR_INVALID and "no report" in str(e.value)
    kib_never = never.get_option("stat_batch_device_kib")
    never.close()
    off = job.configured()
    off.set_window(4)
    off.batch_report_enable(True)
    off.batch_report_enable(False)
    assert [o.tobytes() for o in off.batch_run(job.inputs, RATE, "ieee64", **KW)] == raw
    with pytest.raises(pkg.GdgError) as e:
        off.batch_report()
    assert e.value.code == pkg.GDG_ERR_INVALID
    assert off.get_option("stat_batch_device_kib") == kib_never
    # too little room says so; the counts alone need none
    off.batch_report_enable(True)
    off.batch_run(job.inputs, RATE, "ieee64", **KW)
    import ctypes as C
    ports, blocks = C.c_int(0), C.c_size_t(0)
    assert pkg.lib().gdg_batch_report(off._h, None, 0, C.byref(ports), C.byref(blocks)) == pkg.GDG_OK and (ports.value, blocks.value) == (NCH + 3, BLOCKS)
    few = np.zeros(3, dtype=pkg.BLOCK_STATS_DTYPE)
    assert pkg.lib().gdg_batch_report(off._h, few.ctypes.data, few.size, None, None) == pkg.GDG_ERR_INVALID
    assert "room for 3 records" in pkg.lib().gdg_last_error(off._h).decode()
    off.close()


def sharded(job, slicing, report=True, W=4):
    """shards of 2 + 1 channels, gdg_batch_stream_step_shard plus gdg_batch_finish_master_slice: per slice the shards' results, the
    finished master and the three reports"""
    split = [(0, 2), (2, 1)]
    ctxs = [job.configured(f, n) for f, n in split]
    gens = []
    for g, (ctx, (f, n)) in enumerate(zip(ctxs, split)):
        ctx.set_window(W)
        if report:
            ctx.batch_report_enable()
        it = iter(slicing)
        gens.append(ctx.batch_stream_shard(job.inputs[f:f + n], RATE, "ieee64", lambda left, it=it: next(it), job_samples=job.length, metronome=(g == 0)))
    out = []
    for k in slicing:
        parts = [next(gen) for gen in gens]
        reps = [ctx.batch_report() for ctx in ctxs] if report else None
        master = ctxs[0].batch_finish_master_slice("ieee64", [p[1] for p in parts], [p[2] for p in parts], aux=parts[0][4])
        out.append((parts, master, reps, ctxs[0].batch_report() if report else None))
    for gen in gens:
        assert next(gen, None) is None                              # the job is done: the generator closes it
    for ctx in ctxs:
        ctx.close()
    return out


def test_sharded_job(plain):
    job, dec, raw, rep = plain
    slicing = (2, 3)
    slices = sharded(job, slicing)
    at = 0
    for k, (parts, master, reps, mrep) in zip(slicing, slices):
        assert reps[0].shape == (3, k) and reps[1].shape == (2, k) and mrep.shape == (2, k)
        here = rep[:, at:at + k]
        assert np.concatenate([reps[0][:2], reps[1][:1]]).tobytes() == here[:NCH].tobytes(), "chain outputs: the plain run's records"
        assert reps[0][2].tobytes() == here[NCH + 2].tobytes(), "the metronome, from the shard that runs it"
        assert reps[1][1].tobytes() == np.zeros(k, dtype=rep.dtype).tobytes(), "all-zero records on the shard that does not"
        # the master: (p0 + p1) + aux, the finish's documented association, on the float64 partials the shards handed out
        for side in range(2):
            total = (parts[0][1 + side] + parts[1][1 + side]) + parts[0][4]
            check_records(mrep[side:side + 1], ref_stats(total, BLOCK)[None, :], BLOCK, "master side %d of the slice at block %d" % (side, at))
            assert master[side].tobytes() == total.tobytes()
        at += k
    assert max(m["clipped"].max() for _, _, _, m in slices) > 0
    # the unsliced forms report the same
    whole = sharded(job, (BLOCKS,))[0]
    assert whole[2][0].tobytes() == np.concatenate([s[2][0] for s in slices], axis=1).tobytes()
    assert whole[3].tobytes() == np.concatenate([s[3] for s in slices], axis=1).tobytes()
    pkg = package()
    ctxs = [job.configured(0, 2), job.configured(2, 1)]
    for c in ctxs:
        c.set_window(4)
        c.batch_report_enable()
    res = [c.batch_run_shard(job.inputs[f:f + n], RATE, "ieee64", job_samples=job.length, metronome=(g == 0)) for g, (c, (f, n)) in enumerate(zip(ctxs, [(0, 2), (2, 1)]))]
    assert ctxs[0].batch_report().tobytes() == whole[2][0].tobytes() and ctxs[1].batch_report().tobytes() == whole[2][1].tobytes()
    ctxs[1].batch_finish_master("ieee64", [r[1] for r in res], [r[2] for r in res], aux=res[0][4])
    assert ctxs[1].batch_report().tobytes() == whole[3].tobytes(), "gdg_batch_finish_master: the slice finish's records"
    for c in ctxs:
        c.close()
    assert pkg.BLOCK_STATS_DTYPE == rep.dtype


def test_checkpoint_and_resume(plain):
    job, dec, raw, rep = plain
    blobs = {}
    for with_report in (True, False):
        src = job.configured()
        src.set_window(4)
        if with_report:
            src.batch_report_enable()
        metas, datas, widths = src._stream_split(job.inputs)
        src.batch_stream_open(metas, RATE, "ieee64", **KW)
        need = src.batch_stream_need(2)
        src.batch_stream_step(2, [None if d is None or not c else d[f * w:(f + c) * w] for d, w, (f, c) in zip(datas, widths, need)])
        blobs[with_report] = src.batch_stream_checkpoint()
        src.close()
    assert blobs[True] == blobs[False], "the checkpoint of a job that reports is the checkpoint of one that never did"
    dst = job.configured()
    dst.set_window(4)
    dst.batch_report_enable()                                       # configuration: set again on the target
    metas, datas, widths = dst._stream_split(job.inputs)
    assert dst.batch_stream_resume(metas, RATE, "ieee64", blobs[True], **KW) == 2 * BLOCK
    need = dst.batch_stream_need(3)
    outs = dst.batch_stream_step(3, [None if d is None or not c else d[f * w:(f + c) * w] for d, w, (f, c) in zip(datas, widths, need)])
    got = dst.batch_report()
    dst.batch_stream_close()
    dst.close()
    assert got.tobytes() == np.ascontiguousarray(rep[:, 2:]).tobytes(), "slice 2 of the resumed job: the uninterrupted run's records"
    for r in range(NCH + 3):
        assert outs[r].tobytes() == raw[r][2 * BLOCK * 8:]
