"""The true-peak record of the render report (include/gdg.h, gdg_block_true_peak_rows) on the device.

Stand-alone entry: with the library's own taps handed to the numpy restatement (tests/true_peak_ref.py), all three fields of every record
equal the restatement's exactly -- the bits of true_peak, position, overs: a value is a fixed-order sum over 24 samples, every product
and add rounded on its own, and max is exact.  Rows of 2 * 8192 + r samples for r in {0, 1, 23, 24, 25} (r = 1 and 23: a last block
without any interpolated point; r = 24: exactly one evaluated interval); noise in +-1.2 (overs present), the header's three known answers
against their stated numbers too, silence, two equal crests, a negative crest, non-finite samples; the same block at an odd 8-byte offset
between neighbours of 100.0 behind a guard band of NaN.

Batch runs (3 channels x 4 blocks, channel 1 a reader of channel 0's input behind a small power amp, dither on, LPCM24 out): the records
equal -- on the bytes -- the stand-alone entry's on the float64 rows of the same job rendered to IEEE64, and do not depend on the window,
the slicing, a resume, the source map, the dither or the other three switches; over two shards the chain and metronome ports are equal on
the bytes and the master ports (the finish associates the sums differently) within 1e-12 relative."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import true_peak_ref as ref
from helpers import package, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
RATE = 48000
TAILS = (0, 1, 23, 24, 25)
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def ctx():
    pkg = package()
    pkg.build()
    c = pkg.Context(1, BLOCK)
    yield c
    c.close()


@pytest.fixture(scope="module")
def taps():
    pkg = package()
    pkg.build()
    t = pkg.true_peak_taps()
    t.setflags(write=False)
    return t


def check_exact(ctx, taps, rows, what):
    """every record of the stand-alone entry against the restatement's: all 16 bytes; and never below the sample peak of gdg_block_stats"""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    got = ctx.block_true_peak(rows)
    want = ref.block_true_peak(rows, taps)
    assert got.shape == want.shape == (rows.shape[0], -(-rows.shape[1] // BLOCK))
    for r in range(got.shape[0]):
        for b in range(got.shape[1]):
            g, w = got[r, b], want[r, b]
            print("%s row %d block %d: true_peak %r (want %r) position %d (want %d) overs %d (want %d)" % (
                what, r, b, g["true_peak"], w["true_peak"], g["position"], w["position"], g["overs"], w["overs"]))
            assert g.tobytes() == w.tobytes(), (what, r, b, g, w)
    stats = ctx.block_stats(rows, BLOCK)
    assert np.all(got["true_peak"] >= stats["peak"]), what
    return got


# ---- the stand-alone entry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tail", TAILS)
def test_noise_equals_the_restatement_on_every_bit(ctx, taps, tail):
    rng = np.random.default_rng(40 + tail)
    rows = rng.uniform(-1.2, 1.2, (3, 2 * BLOCK + tail))
    got = check_exact(ctx, taps, rows, "noise, tail %d" % tail)
    assert np.all(got["overs"][:, :2] > 0), "noise in +-1.2 has interpolated points above 1"
    if tail:
        last = got[:, 2]
        if tail < 24:                                                # no interpolated point: the samples' own peak at a sample's position, no overs
            assert np.all(last["overs"] == 0) and np.all(last["position"] % 4 == 0)
            assert np.all(last["true_peak"] == np.max(np.abs(rows[:, 2 * BLOCK:]), axis=1))
        if tail == 24:                                               # exactly one evaluated interval: positions 4 * 11 + 1 .. 3 are the only odd ones
            assert np.all((last["position"] % 4 == 0) | ((last["position"] >= 45) & (last["position"] <= 47)))


@pytest.mark.parametrize("tail", TAILS)
def test_known_answers(ctx, taps, tail):
    n = 2 * BLOCK + tail
    impulse = np.zeros(n)
    impulse[4000] = 1.0
    dc = np.full(n, 0.5)
    sine = 0.9 * np.sin(2 * np.pi * np.arange(n) / 4 + np.pi / 4)
    silent = np.zeros(n)
    silent[BLOCK:2 * BLOCK] = -0.0
    crests = np.zeros(n)
    crests[[1000, 5000, BLOCK + 30, BLOCK + 8000]] = 0.75, 0.75, -0.5, -0.5          # two equal crests per block; negative ones in block 1
    negative = np.zeros(n)
    negative[[777, BLOCK + 12]] = -0.875
    got = check_exact(ctx, taps, np.stack([impulse, dc, sine, silent, crests, negative]), "known answers, tail %d" % tail)
    g = got[0, 0]
    assert (g["true_peak"], g["position"], g["overs"]) == (1.0, 16000, 0), "the impulse: exact"
    assert got[0, 1].tobytes() == bytes(16)
    for b in range(got.shape[1]):
        if b < 2 or tail >= 24:
            assert 0.5 <= got[1, b]["true_peak"] <= 0.5 * (1 + 24 * EPS) and got[1, b]["overs"] == 0, "the constant: the stated interval"
        else:
            assert got[1, b]["true_peak"] == 0.5 and got[1, b]["position"] == 0
    for b in range(2):
        assert abs(got[2, b]["true_peak"] - 0.900330) <= 1e-6 and got[2, b]["position"] % 4 == 2 and got[2, b]["overs"] == 0, "the sine at fs/4"
    assert abs(ctx.block_stats(sine[None, :], BLOCK)[0, 0]["peak"] - 0.636396) <= 1e-6
    assert got[3].tobytes() == bytes(16 * got.shape[1]), "an all-zero block (of +0.0 or of -0.0): true_peak 0, position 0, overs 0"
    assert (got[4, 0]["true_peak"], got[4, 0]["position"]) == (0.75, 4000) and (got[4, 1]["true_peak"], got[4, 1]["position"]) == (0.5, 120), "the lower position wins"
    assert (got[5, 0]["true_peak"], got[5, 0]["position"]) == (0.875, 4 * 777) and (got[5, 1]["true_peak"], got[5, 1]["position"]) == (0.875, 48)


def test_a_negative_inter_sample_crest(ctx, taps):
    """two neighbouring samples of -0.7: the crest lies half-way between them, at -0.7 * 2 * 0.633825 = -0.887; the record holds its magnitude"""
    x = np.zeros(BLOCK)
    x[[4000, 4001]] = -0.7
    got = check_exact(ctx, taps, x, "a negative crest")[0, 0]
    assert got["position"] == 4 * 4000 + 2 and abs(got["true_peak"] - 0.7 * 2 * 0.633825) <= 1e-6 and got["overs"] == 0
    _, v = ref.points(x, taps)
    assert v[1][4000 - (ref.H - 1)] == -got["true_peak"]


def device_records(ctx, stored, offset, stride, n_rows, samples):
    """gdg_block_true_peak_rows_device on rows `stride` samples apart from sample `offset` of the flat array `stored`"""
    pkg = package()
    n = n_rows * -(-samples // BLOCK) * 2
    d_in, d_out = pkg.DeviceBuffer(ctx, 1, stored.size), pkg.DeviceBuffer(ctx, 1, n + 4)
    try:
        d_in.upload(stored)
        d_out.upload(np.full(n + 4, -7.0))
        ctx.block_true_peak_device(d_in.ptr + 8 * offset, stride, n_rows, samples, d_out.ptr)
        ctx.synchronize()
        raw = d_out.download().reshape(-1)
        assert np.all(raw[n:] == -7.0), "a record was written past the last one"
        return raw[:n].copy().view(ref.DTYPE).reshape(n_rows, -1)
    finally:
        d_in.free()
        d_out.free()


@pytest.mark.parametrize("samples", [BLOCK, BLOCK + 25])
def test_statelessness_alignment_and_guard_band(ctx, taps, samples):
    """the same row at a 16-byte aligned place (pair loads) and at an odd 8-byte offset (single loads), between neighbours filled with
    100.0, behind a guard band of NaN: the same 16 bytes per record, and nothing of the neighbours or the guard in any of them"""
    rng = np.random.default_rng(9)
    row = rng.uniform(-1.2, 1.2, samples)
    host = ctx.block_true_peak(row)
    assert host.tobytes() == ref.block_true_peak([row], taps).tobytes()
    stride = samples + (samples & 1)                                 # even: the launcher may take pairs when the row's start allows it
    for flank in (40, 41):                                           # the row starts at sample 104 (16-byte aligned) or 105 (8 bytes past)
        start = 64 + flank
        stored = np.full(start + stride + flank + 64, np.nan)        # the guard band at either end
        stored[64:start] = 100.0
        stored[start:start + samples] = row
        stored[start + samples:start + samples + flank] = 100.0
        dev = device_records(ctx, stored, start, stride, 1, samples)
        assert np.all(np.isfinite(dev["true_peak"])) and dev.tobytes() == host.tobytes(), "row at sample %d" % start
    if samples == BLOCK:                                             # a block's record does not depend on its place in the row either
        got = ctx.block_true_peak(np.concatenate([np.full(BLOCK, 100.0), row, np.full(BLOCK, 100.0)]))
        assert got[0, 1].tobytes() == host[0, 0].tobytes() and got[0, 0]["true_peak"] >= 100.0
    two = np.stack([row, row[::-1]])                                 # an odd `samples` puts the second row 8 bytes past a 16-byte boundary
    assert ctx.block_true_peak(two)[0].tobytes() == host[0].tobytes()


def test_non_finite_samples_count_as_zero(ctx, taps):
    rng = np.random.default_rng(6)
    x = rng.uniform(-1.0, 1.0, BLOCK + 30)
    z, bad = x.copy(), x.copy()
    at = [0, 77, 4097, BLOCK - 1, BLOCK + 5, BLOCK + 29]
    z[at] = 0.0
    bad[at] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
    a, b = ctx.block_true_peak(z), ctx.block_true_peak(bad)
    assert a.tobytes() == b.tobytes() and np.all(np.isfinite(b["true_peak"]))
    assert b.tobytes() == ref.block_true_peak([bad], taps).tobytes()
    allbad = np.full(100, np.nan)
    assert ctx.block_true_peak(allbad).tobytes() == bytes(16)


def test_refusals_of_the_stand_alone_entry(ctx):
    pkg = package()
    lib = pkg.lib()
    row = np.zeros(16)
    ptrs = (C.c_void_p * 1)(row.ctypes.data)
    none = (C.c_void_p * 1)(None)
    rec = np.zeros(1, dtype=pkg.BLOCK_TRUE_PEAK_DTYPE)
    for rc in (lib.gdg_block_true_peak_rows(ctx._h, None, 1, 16, rec.ctypes.data),                      # no rows
               lib.gdg_block_true_peak_rows(ctx._h, none, 1, 16, rec.ctypes.data),                      # a NULL row
               lib.gdg_block_true_peak_rows(ctx._h, ptrs, 1, 16, None),                                 # no records
               lib.gdg_block_true_peak_rows(ctx._h, ptrs, 0, 16, rec.ctypes.data),                      # n_rows <= 0
               lib.gdg_block_true_peak_rows(ctx._h, ptrs, -1, 16, rec.ctypes.data),
               lib.gdg_block_true_peak_rows_device(ctx._h, None, 8, 1, 8, 8),
               lib.gdg_block_true_peak_rows_device(ctx._h, 8, 8, 1, 8, None),
               lib.gdg_block_true_peak_rows_device(ctx._h, 8, 8, 0, 8, 8),
               lib.gdg_block_true_peak_rows_device(ctx._h, 8, 4, 2, 8, 8),                               # stride < samples
               lib.gdg_block_true_peak_rows_device(ctx._h, 12, 8, 2, 8, 8)):                             # a 4-byte aligned row
        assert rc == pkg.GDG_ERR_INVALID and lib.gdg_last_error(ctx._h)
    assert ctx.block_true_peak(np.zeros((2, 16))).shape == (2, 1)    # the context stays usable


# ---- batch runs --------------------------------------------------------------------------------------------------------------------
NCH, BLOCKS = 3, 4
KW = dict(metronome_to_master=True)
FIR = np.array([0.0, 0.0, 0.0, 0.0, 0.0, -0.9, 0.1])
POSITIONS = [(-35.0, 0.6, 1.0), (40.0, 0.8, 0.9), (5.0, 0.7, 0.8)]
SOURCES = [0, 0, 2]                                                  # channel 1 reads channel 0's input
EDGES = [100.0, 1000.0, 10000.0]
REFS = [0, 0, 0, 0, 3, 5]
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

    def configured(first=0, count=NCH, true_peak=True, report=False, edges=None, refs=None, dither=True, sources=True):
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
        if sources:
            ctx.batch_set_sources([s - first for s in SOURCES[first:first + count]])
        if dither:
            ctx.batch_set_dither(1, seed=99, port_base=first)
        if true_peak:
            ctx.batch_true_peak_enable()
        if report:
            ctx.batch_report_enable()
        if edges is not None:
            ctx.batch_spectrum_enable(edges)
        if refs is not None:
            ctx.batch_align_enable(refs, 64)
        return ctx

    _job["job"] = SimpleNamespace(inputs=inputs, configured=configured, length=n, x0=x0)
    return _job["job"]


def one_call(job, fmt="lpcm24", W=2, inputs=None, **cfg):
    ctx = job.configured(**cfg)
    ctx.set_window(W)
    res = ctx.batch_run(job.inputs if inputs is None else inputs, RATE, fmt, **KW)
    rec = ctx.batch_true_peak()
    ctx.close()
    return [o.tobytes() for o in res], rec


@pytest.fixture(scope="module")
def plain():
    package().build()
    job = the_job()
    raw, rec = one_call(job)
    rec.setflags(write=False)
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
        recs.append(ctx.batch_true_peak())
        assert recs[-1].shape == (NCH + 3, k)
    ctx.batch_stream_close()
    ctx.close()
    return [b"".join(p[r].tobytes() for p in parts) for r in range(NCH + 3)], np.concatenate(recs, axis=1)


def test_batch_equals_the_stand_alone_entry_on_the_float64_rows(plain, ctx, taps):
    job, raw, rec = plain
    assert rec.shape == (NCH + 3, BLOCKS) and rec.dtype.itemsize == 16
    raw64, rec64 = one_call(job, "ieee64")
    rows = np.stack([np.frombuffer(b, dtype="<f8") for b in raw64])
    alone = ctx.block_true_peak(rows)
    assert rec.tobytes() == alone.tobytes(), "LPCM24 job, dither on: the records of the float64 rows, in the order of out_bytes"
    assert rec64.tobytes() == alone.tobytes()
    assert alone.tobytes() == ref.block_true_peak(rows, taps).tobytes()
    assert np.all(rec["true_peak"][:NCH] > 0.0) and np.any(rec["position"] % 4 != 0), "some block's peak lies between two samples"


def test_records_do_not_depend_on_window_or_slicing(plain):
    job, raw, rec = plain
    for W in (1, 2, 4):                                              # 4: the whole job in one window
        raw_w, rec_w = one_call(job, W=W)
        assert rec_w.tobytes() == rec.tobytes() and raw_w == raw, "one call, window %d" % W
    for W in (1, 2):
        for slicing in ((1, 1, 1, 1), (3, 1), (1, 2, 1)):
            raw_s, rec_s = streamed(job, slicing, W)
            assert rec_s.tobytes() == rec.tobytes() and raw_s == raw, "slices %r, window %d" % (slicing, W)


def test_records_of_a_sharded_job(plain, ctx, taps):
    """channels 0 and 1 (a root and its reader) on one shard context, channel 2 on another, the master finished per slice: chain and
    metronome ports on the bytes; the master's true_peak within 1e-12 relative (the finish associates the sums differently), its position
    equal wherever the restatement's runner-up stands 1 % below the maximum"""
    job, raw, rec = plain
    slicing = (1, 3)
    ctxs = [job.configured(0, 2), job.configured(2, 1)]
    gens = []
    for g, (c, (f, n)) in enumerate(zip(ctxs, ((0, 2), (2, 1)))):
        it = iter(slicing)
        gens.append(c.batch_stream_shard(job.inputs[f:f + n], RATE, "lpcm24", lambda left, it=it: next(it), job_samples=job.length, metronome=(g == 0)))
    raw64 = one_call(job, "ieee64")[0]
    master_rows = [np.frombuffer(raw64[NCH + s], dtype="<f8") for s in range(2)]
    at = 0
    for k in slicing:
        parts = [next(gen) for gen in gens]
        recs = [c.batch_true_peak() for c in ctxs]
        assert recs[0].shape == (3, k) and recs[1].shape == (2, k)
        here = rec[:, at:at + k]
        assert recs[0][0].tobytes() == here[0].tobytes() and recs[0][1].tobytes() == here[1].tobytes() and recs[1][0].tobytes() == here[2].tobytes(), "chain outputs"
        assert recs[0][2].tobytes() == here[NCH + 2].tobytes(), "the metronome, from the shard that runs it"
        assert recs[1][1].tobytes() == bytes(16 * k), "all-zero on the shard that does not"
        ctxs[1].batch_finish_master_slice("lpcm24", [p[1] for p in parts], [p[2] for p in parts], aux=parts[0][4], sample_rate=RATE)
        m = ctxs[1].batch_true_peak()
        assert m.shape == (2, k)
        for s in range(2):
            want = here[NCH + s]
            print("master side %d: true_peak %r (plain %r)" % (s, m[s]["true_peak"], want["true_peak"]))
            assert np.all(np.abs(m[s]["true_peak"] - want["true_peak"]) <= 1e-12 * want["true_peak"]) and np.all(m[s]["overs"] == want["overs"])
            for b in range(k):
                if ref.runner_up(master_rows[s][(at + b) * BLOCK:(at + b + 1) * BLOCK], taps) <= 0.99:
                    assert m[s][b]["position"] == want[b]["position"], (s, b)
            # ... and exactly the stand-alone entry's on the sums the finish made: (p0 + p1) + aux
            total = (parts[0][1 + s] + parts[1][1 + s]) + parts[0][4]
            assert m[s].tobytes() == ctx.block_true_peak(total)[0].tobytes()
        at += k
    for gen in gens:
        assert next(gen, None) is None
    for c in ctxs:
        c.close()


def test_records_across_a_checkpoint(plain):
    job, raw, rec = plain
    src = job.configured(sources=False)
    inputs = [job.inputs[0], job.inputs[0], job.inputs[2]]           # the source map spelled out: a checkpoint does not record shared sources
    whole_raw, whole = one_call(job, inputs=inputs, sources=False)
    assert whole.tobytes() == rec.tobytes() and whole_raw == raw, "a source map changes no record: the reader renders what its own copy would"
    metas, datas, widths = src._stream_split(inputs)
    src.batch_stream_open(metas, RATE, "lpcm24", **KW)
    src.batch_stream_step(1, slice_inputs(datas, widths, src.batch_stream_need(1)))
    first = src.batch_true_peak()
    blob = src.batch_stream_checkpoint()
    src.close()
    never = job.configured(sources=False, true_peak=False)
    never.batch_stream_open(metas, RATE, "lpcm24", **KW)
    never.batch_stream_step(1, slice_inputs(datas, widths, never.batch_stream_need(1)))
    assert never.batch_stream_checkpoint() == blob, "the checkpoint of a job that takes the true peak is the checkpoint of one that never did"
    never.close()
    dst = job.configured(sources=False)                              # a fresh context, the switch set again
    assert dst.batch_stream_resume(metas, RATE, "lpcm24", blob, **KW) == BLOCK
    outs = dst.batch_stream_step(3, slice_inputs(datas, widths, dst.batch_stream_need(3)))
    got = dst.batch_true_peak()
    dst.batch_stream_close()
    dst.close()
    assert np.concatenate([first, got], axis=1).tobytes() == rec.tobytes()
    for r in range(NCH + 3):
        assert outs[r].tobytes() == raw[r][BLOCK * 3:]


def test_switches(plain):
    pkg = package()
    job, raw, rec = plain
    run = lambda c: [o.tobytes() for o in c.batch_run(job.inputs, RATE, "lpcm24", **KW)]
    # the parent's state: the switch never touched
    never = job.configured(true_peak=False, report=True, edges=EDGES, refs=REFS)
    assert run(never) == raw, "the true peak changes no output byte"
    rep, bands, al = never.batch_report(), never.batch_spectrum(), never.batch_align()
    kib = never.get_option("stat_batch_device_kib")
    with pytest.raises(pkg.GdgError) as e:
        never.batch_true_peak()
    assert e.value.code == pkg.GDG_ERR_INVALID and "no true-peak records" in str(e.value)
    never.close()
    # switched on and off again: the parent's bytes, device memory, report, bands and alignment records
    off = job.configured(true_peak=True, report=True, edges=EDGES, refs=REFS)
    off.batch_true_peak_enable(False)
    assert run(off) == raw
    assert off.batch_report().tobytes() == rep.tobytes() and off.batch_spectrum().tobytes() == bands.tobytes() and off.batch_align().tobytes() == al.tobytes()
    assert off.get_option("stat_batch_device_kib") == kib
    with pytest.raises(pkg.GdgError):
        off.batch_true_peak()
    off.close()
    # all four on: each of them what it is alone (`plain` is the true peak alone); only a half of `enc` grows, by 16 + ports x W x 16 bytes
    four = job.configured(report=True, edges=EDGES, refs=REFS)
    assert run(four) == raw
    assert four.batch_true_peak().tobytes() == rec.tobytes() and four.batch_report().tobytes() == rep.tobytes()
    assert four.batch_spectrum().tobytes() == bands.tobytes() and four.batch_align().tobytes() == al.tobytes()
    grown = four.get_option("stat_batch_device_kib") - kib
    want = 2 * (16 + (NCH + 3) * 2 * 16)                             # two halves, W = 2: 416 bytes, which the option counts in KiB
    assert 0 <= grown <= -(-want // 1024), "two halves of enc grow by %d bytes, nothing else does: %d KiB" % (want, grown)
    four.close()
    for cfg in (dict(report=True), dict(edges=EDGES), dict(refs=REFS)):
        raw_s, rec_s = streamed(job, (2, 2), 2, **cfg)
        assert raw_s == raw and rec_s.tobytes() == rec.tobytes()
    # dither off: other bytes, the same records (the rows are read before the dither)
    raw_d, rec_d = one_call(job, dither=False)
    assert rec_d.tobytes() == rec.tobytes() and raw_d != raw


def test_refusals(plain):
    pkg = package()
    job, raw, rec = plain
    lib = pkg.lib()
    c = job.configured(true_peak=False)
    with pytest.raises(pkg.GdgError, match="no true-peak records"):
        c.batch_true_peak()                                          # before any call has completed
    c.batch_true_peak_enable()
    with pytest.raises(pkg.GdgError, match="no true-peak records"):
        c.batch_true_peak()                                          # enabled, and still no call
    # while a streamed job is open the switch is refused and nothing changes
    metas, datas, widths = c._stream_split(job.inputs)
    c.batch_stream_open(metas, RATE, "lpcm24", **KW)
    assert lib.gdg_batch_true_peak_enable(c._h, 0) == pkg.GDG_ERR_INVALID and b"streamed batch run is open" in lib.gdg_last_error(c._h)
    assert lib.gdg_batch_true_peak_enable(c._h, 1) == pkg.GDG_ERR_INVALID
    outs = c.batch_stream_step(BLOCKS, slice_inputs(datas, widths, c.batch_stream_need(BLOCKS)))
    assert c.batch_true_peak().tobytes() == rec.tobytes() and [o.tobytes() for o in outs] == raw
    c.batch_stream_close()
    # too little room says so, with the counts; NULL gives the counts alone
    ports, blocks = C.c_int(0), C.c_size_t(0)
    few = np.zeros(5, dtype=pkg.BLOCK_TRUE_PEAK_DTYPE)
    assert lib.gdg_batch_true_peak(c._h, few.ctypes.data, few.size, C.byref(ports), C.byref(blocks)) == pkg.GDG_ERR_INVALID
    assert (ports.value, blocks.value) == (NCH + 3, BLOCKS) and b"room for 5 records" in lib.gdg_last_error(c._h)
    assert lib.gdg_batch_true_peak(c._h, None, 0, C.byref(ports), C.byref(blocks)) == pkg.GDG_OK
    c.close()
