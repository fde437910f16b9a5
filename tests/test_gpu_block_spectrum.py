"""The band spectrum of the render report (include/gdg.h, gdg_block_spectrum_rows) on the device.

Stand-alone entry: against the numpy restatement (tests/spectrum_ref.py) within 1e-12 * T per block and band, T = the restatement's sum
over all bins of that block -- a 13-stage float64 transform errs by a few 1e-15 of ||X||, a band's power then by at most twice that
times T; 1e-12 leaves two orders of margin.  Empty bands and all-zero blocks exactly 0.0; nothing outside a row is read; the same
samples give the same bits at any alignment; a non-finite sample counts as 0.

Batch runs (2 channels x 3 blocks, one input resampled, overdrive -> small power amp on channel 1, master and metronome, LPCM24 out):
the bands equal -- on the bytes -- the stand-alone entry's on the float64 rows of the same job rendered to IEEE64, and do not depend on
the window, the slicing, the sharding, a resume, the source map or the dither."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import spectrum_ref as ref
from helpers import package, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
RATE = 48000
# ten octave edges from 22.1 Hz, then Nyquist and beyond: [.., 24000) ends at bin 4095, [24000, 30000) holds bin 4096 alone, [30000, 60000) no bin
EDGES = [22.1 * 2.0 ** i for i in range(10)] + [24000.0, 30000.0, 60000.0]


def close_to_ref(got, rows, rate, edges, what):
    """|got - ref| <= 1e-12 * T per block and band; a band without a bin exactly 0.0"""
    lo = ref.k_lo(edges, rate)
    empty = lo[1:] == lo[:-1]
    worst = 0.0
    for r, row in enumerate(rows):
        want, tot = ref.block_spectrum(row, rate, edges)
        assert got[r].shape == want.shape, what
        for j in range(want.shape[0]):
            err = np.abs(got[r, j] - want[j])
            if tot[j] > 0.0:
                worst = max(worst, float(err.max() / tot[j]))
            assert np.all(err <= 1e-12 * tot[j]), "%s: row %d block %d: %s against %s (T = %r)" % (what, r, j, got[r, j], want[j], tot[j])
            assert np.all(got[r, j][empty] == 0.0), "%s: a band without a bin is exactly 0.0" % what
    print("%s: worst |got - ref| / T = %.3e" % (what, worst))


@pytest.fixture(scope="module")
def ctx():
    pkg = package()
    pkg.build()
    c = pkg.Context(1, BLOCK)
    yield c
    c.close()


def device_bands(ctx, stored, offset, stride, n_rows, samples, rate, edges):
    """gdg_block_spectrum_rows_device on rows `stride` samples apart from sample `offset` of the flat array `stored`"""
    pkg = package()
    n = n_rows * -(-samples // BLOCK) * (len(edges) - 1)
    d_in, d_out = pkg.DeviceBuffer(ctx, 1, stored.size), pkg.DeviceBuffer(ctx, 1, n + 4)
    try:
        d_in.upload(stored)
        d_out.upload(np.full(n + 4, -7.0))
        ctx.block_spectrum_device(d_in.ptr + 8 * offset, stride, n_rows, samples, rate, edges, d_out.ptr)
        ctx.synchronize()
        raw = d_out.download().reshape(-1)
        assert np.all(raw[n:] == -7.0), "a band was written past the last one"
        return raw[:n].copy().reshape(n_rows, -1, len(edges) - 1)
    finally:
        d_in.free()
        d_out.free()


# ---- the stand-alone entry ---------------------------------------------------------------------------------------------------------
def test_rows_against_the_restatement(ctx):
    samples = 2 * BLOCK + 100                                        # the last block is short
    t = np.arange(samples)
    rng = np.random.default_rng(11)
    rows = np.stack([0.3 * rng.standard_normal(samples),
                     0.5 * np.sin(2.0 * np.pi * 100.0 * t / BLOCK),                                 # bin-centred
                     0.4 * np.sin(2.0 * np.pi * 1234.567 * t / RATE + 0.3) + 0.2])                  # off-bin, plus DC
    got = ctx.block_spectrum(rows, RATE, EDGES)
    assert got.shape == (3, 3, len(EDGES) - 1)
    close_to_ref(got, rows, RATE, EDGES, "host form")
    assert np.all(got[:, :, -1] == 0.0) and np.all(got[0, :, :-1] > 0.0)
    # the known answer on the device: bins 99, 100, 101 of the bin-centred sine in bands of their own
    hz = lambda k: k * RATE / 8192.0
    three = ctx.block_spectrum(rows[1, :BLOCK], RATE, [hz(98.5), hz(99.5), hz(100.5), hz(101.5)])[0, 0]
    assert np.all(np.abs(three - np.array([0.25 / 12, 0.25 / 3, 0.25 / 12])) <= 1e-12 * 0.125), three
    # 32 bands, other rates
    for rate in (44100, 192000):
        edges = [0.0] + [15.0 * 1.27 ** i for i in range(32)]
        close_to_ref(ctx.block_spectrum(rows[:, :BLOCK + 1], rate, edges), rows[:, :BLOCK + 1], rate, edges, "33 edges at %d Hz" % rate)
    # an all-zero block: exactly 0.0 everywhere (also -0.0 samples)
    z = np.zeros((2, 2 * BLOCK))
    z[1, :] = -0.0
    z[0, BLOCK:] = rows[0, :BLOCK]
    gz = ctx.block_spectrum(z, RATE, EDGES)
    assert np.all(gz[0, 0] == 0.0) and np.all(gz[1] == 0.0) and np.all(np.signbit(gz[:, 0]) == False)
    assert gz[0, 1].tobytes() == got[0, 0].tobytes(), "block 1 of another row: the bits of block 0"
    assert ctx.block_spectrum(np.zeros((2, 0)), RATE, EDGES).shape == (2, 0, len(EDGES) - 1)


def test_nothing_outside_the_row_is_read_and_alignment_changes_no_bit(ctx):
    samples = BLOCK + 100
    rng = np.random.default_rng(12)
    row = rng.uniform(-1.0, 1.0, samples)
    host = ctx.block_spectrum(row, RATE, EDGES)
    for offset in (4, 5):                                            # 16-byte aligned (pair loads), 8 bytes past a 16-byte boundary (single loads)
        stored = np.full(offset + samples + 8192 + 11, np.nan)
        stored[offset:offset + samples] = row
        dev = device_bands(ctx, stored, offset, samples + 4, 1, samples, RATE, EDGES)
        assert np.all(np.isfinite(dev)), "offset %d: a sample outside the row was read" % offset
        assert dev.tobytes() == host.tobytes(), "offset %d" % offset
    # two rows an odd stride apart: row 1 lies 8 bytes past a 16-byte boundary
    stride = samples + 1
    stored = np.full(2 * stride + 6, np.nan)
    stored[:samples], stored[stride:stride + samples] = row, row
    dev = device_bands(ctx, stored, 0, stride, 2, samples, RATE, EDGES)
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[0].tobytes()


def test_non_finite_samples_count_as_zero(ctx):
    rng = np.random.default_rng(13)
    x = rng.uniform(-1.0, 1.0, BLOCK)
    y = x.copy()
    y[77], y[4097] = np.nan, np.inf
    x[77] = x[4097] = 0.0
    a, b = ctx.block_spectrum(x, RATE, EDGES), ctx.block_spectrum(y, RATE, EDGES)
    assert np.all(np.isfinite(b)) and a.tobytes() == b.tobytes()
    y[4097] = -np.inf
    assert ctx.block_spectrum(y, RATE, EDGES).tobytes() == a.tobytes()


def test_refusals(ctx):
    pkg = package()
    e = np.array(EDGES)
    rev = e[::-1].copy()
    lib = pkg.lib()
    for rc in (lib.gdg_block_spectrum_rows_device(ctx._h, 8, 4, 1, 8, RATE, e.ctypes.data, e.size, 8),         # stride < samples
               lib.gdg_block_spectrum_rows_device(ctx._h, 12, 8, 1, 8, RATE, e.ctypes.data, e.size, 8),        # a 4-byte aligned row
               lib.gdg_block_spectrum_rows_device(ctx._h, 8, 8, 1, 8, 0, e.ctypes.data, e.size, 8),            # no rate
               lib.gdg_block_spectrum_rows_device(ctx._h, 8, 8, 1, 8, RATE, e.ctypes.data, 1, 8),              # one edge
               lib.gdg_block_spectrum_rows_device(ctx._h, 8, 8, 1, 8, RATE, rev.ctypes.data, e.size, 8),
               lib.gdg_block_spectrum_rows_device(ctx._h, 8, 8, 1, 8, RATE, None, 2, 8)):
        assert rc == pkg.GDG_ERR_INVALID


# ---- batch runs --------------------------------------------------------------------------------------------------------------------
NCH, BLOCKS = 2, 3
KW = dict(metronome_to_master=True)
FIR = np.array([0.8, 0.3, -0.2, 0.1])
POSITIONS = [(-35.0, 0.6, 1.0), (40.0, 0.8, 0.9)]
_job = {}


def the_job():
    """channel 0: an empty chain fed at the job's rate; channel 1: overdrive -> a small power amp, its input at 44.1 kHz (resampled);
    a quiet metronome in the master"""
    if "job" in _job:
        return _job["job"]
    pkg = package()
    n = BLOCKS * BLOCK
    x0 = 0.4 * synth_signal(0, n, RATE)
    x1 = 0.5 * synth_signal(7, 22000, 44100)                         # covers 23947 of the job's 24576 samples
    tick, tock = 0.008 * np.sin(np.arange(600) * 0.2), 0.006 * np.sin(np.arange(400) * 0.3)
    enc = lambda x: np.frombuffer(np.asarray(x, dtype="<f8").tobytes(), dtype=np.uint8)
    inputs = [(enc(x0), "ieee64", RATE), (enc(x1), "ieee64", 44100)]

    def configured(first=0, count=NCH, edges=EDGES, report=False):
        ctx = pkg.Context(count, BLOCK)
        if first <= 1 < first + count:
            ctx.append_unit(1 - first, "overdrive", params=[0, 15, 80, -3, 1, 0])
            ctx.append_unit(1 - first, "power_amp", fir=FIR)
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(count):
            ctx.spatializer_set_position(c, *POSITIONS[first + c])
        ctx.metronome_set_sounds(tick, tock)
        ctx.metronome_configure(3, 200, RATE)
        ctx.set_window(2)
        if edges is not None:
            ctx.batch_spectrum_enable(edges)
        if report:
            ctx.batch_report_enable()
        return ctx

    _job["job"] = SimpleNamespace(inputs=inputs, configured=configured, length=n)
    return _job["job"]


def one_call(job, fmt="lpcm24", W=2, inputs=None, **cfg):
    ctx = job.configured(**cfg)
    ctx.set_window(W)
    res = ctx.batch_run(job.inputs if inputs is None else inputs, RATE, fmt, **KW)
    spec = ctx.batch_spectrum()
    ctx.close()
    return [o.tobytes() for o in res], spec


@pytest.fixture(scope="module")
def plain():
    package().build()
    job = the_job()
    raw, spec = one_call(job)
    return job, raw, spec


def slice_inputs(datas, widths, need):
    return [None if d is None or not c else d[f * w:(f + c) * w] for d, w, (f, c) in zip(datas, widths, need)]


def test_batch_equals_the_stand_alone_entry_on_the_float64_rows(plain, ctx):
    job, raw, spec = plain
    assert spec.shape == (NCH + 3, BLOCKS, len(EDGES) - 1)
    raw64, spec64 = one_call(job, "ieee64")
    rows = np.stack([np.frombuffer(b, dtype="<f8") for b in raw64])  # the N chain outputs, master left, master right, metronome
    assert rows.shape == (NCH + 3, job.length)
    alone = ctx.block_spectrum(rows, RATE, EDGES)
    assert spec.tobytes() == alone.tobytes(), "LPCM24 job: the bands of the float64 rows, in the order of out_bytes"
    assert spec64.tobytes() == alone.tobytes()
    close_to_ref(spec, rows, RATE, EDGES, "batch run")
    assert all(spec[p].sum() > 0.0 for p in range(NCH + 3)) and len({spec[p].tobytes() for p in range(NCH + 3)}) == NCH + 3
    # a NULL entry in out_bytes changes nothing
    c = job.configured()
    metas, datas, widths = c._stream_split(job.inputs)
    c.batch_stream_open(metas, RATE, "lpcm24", **KW)
    outs = [None if r in (0, NCH) else np.zeros(job.length * 3, dtype=np.uint8) for r in range(NCH + 3)]
    res = c.batch_stream_step(BLOCKS, slice_inputs(datas, widths, c.batch_stream_need(BLOCKS)), outs=outs)
    assert c.batch_spectrum().tobytes() == spec.tobytes() and res[1].tobytes() == raw[1] and res[NCH + 1].tobytes() == raw[NCH + 1]
    c.batch_stream_close()
    c.close()


def streamed(job, slicing, W, **cfg):
    ctx = job.configured(**cfg)
    ctx.set_window(W)
    metas, datas, widths = ctx._stream_split(job.inputs)
    ctx.batch_stream_open(metas, RATE, "lpcm24", **KW)
    parts, specs = [], []
    for k in slicing:
        parts.append(ctx.batch_stream_step(k, slice_inputs(datas, widths, ctx.batch_stream_need(k))))
        specs.append(ctx.batch_spectrum())
        assert specs[-1].shape == (NCH + 3, k, len(EDGES) - 1)
    ctx.batch_stream_close()
    ctx.close()
    return [b"".join(p[r].tobytes() for p in parts) for r in range(NCH + 3)], np.concatenate(specs, axis=1)


def test_bands_do_not_depend_on_window_or_slicing(plain):
    job, raw, spec = plain
    for W in (1, 2):
        raw_w, spec_w = one_call(job, W=W)
        assert spec_w.tobytes() == spec.tobytes() and raw_w == raw, "one call, window %d" % W
        raw_s, spec_s = streamed(job, (1, 2), W)
        assert spec_s.tobytes() == spec.tobytes() and raw_s == raw, "slices of 1 + 2 blocks, window %d" % W


def test_bands_of_a_sharded_job(plain):
    """two shard contexts on one device plus gdg_batch_finish_master_slice: chain and metronome ports on the bytes, the master -- whose
    sums are associated differently -- within 1e-12 * T of the plain run's"""
    job, raw, spec = plain
    slicing = (1, 2)
    ctxs = [job.configured(0, 1), job.configured(1, 1)]
    gens = []
    for g, c in enumerate(ctxs):
        it = iter(slicing)
        gens.append(c.batch_stream_shard(job.inputs[g:g + 1], RATE, "lpcm24", lambda left, it=it: next(it), job_samples=job.length, metronome=(g == 0)))
    at = 0
    raw64 = one_call(job, "ieee64")[0]
    master_rows = [np.frombuffer(raw64[NCH + s], dtype="<f8") for s in range(2)]
    for k in slicing:
        parts = [next(gen) for gen in gens]
        specs = [c.batch_spectrum() for c in ctxs]
        assert specs[0].shape == (2, k, len(EDGES) - 1) and specs[1].shape == (2, k, len(EDGES) - 1)
        here = spec[:, at:at + k]
        assert specs[0][0].tobytes() == here[0].tobytes() and specs[1][0].tobytes() == here[1].tobytes(), "chain outputs"
        assert specs[0][1].tobytes() == here[NCH + 2].tobytes(), "the metronome, from the shard that runs it"
        assert np.all(specs[1][1] == 0.0), "all-zero on the shard that does not"
        ctxs[1].batch_finish_master_slice("lpcm24", [p[1] for p in parts], [p[2] for p in parts], aux=parts[0][4], sample_rate=RATE)
        m = ctxs[1].batch_spectrum()
        assert m.shape == (2, k, len(EDGES) - 1)
        for s in range(2):
            _, tot = ref.block_spectrum(master_rows[s][at * BLOCK:(at + k) * BLOCK], RATE, EDGES)
            assert np.all(np.abs(m[s] - here[NCH + s]) <= 1e-12 * tot[:, None]), "master side %d" % s
            # ... and exactly the stand-alone entry's on the sums the finish made: (p0 + p1) + aux
            total = (parts[0][1 + s] + parts[1][1 + s]) + parts[0][4]
            assert m[s].tobytes() == ctxs[1].block_spectrum(total, RATE, EDGES)[0].tobytes()
        at += k
    for gen in gens:
        assert next(gen, None) is None
    for c in ctxs:
        c.close()


def test_bands_across_a_checkpoint(plain):
    job, raw, spec = plain
    src = job.configured()
    metas, datas, widths = src._stream_split(job.inputs)
    src.batch_stream_open(metas, RATE, "lpcm24", **KW)
    src.batch_stream_step(1, slice_inputs(datas, widths, src.batch_stream_need(1)))
    first = src.batch_spectrum()
    blob = src.batch_stream_checkpoint()
    src.close()
    never = job.configured(edges=None)
    never.batch_stream_open(metas, RATE, "lpcm24", **KW)
    never.batch_stream_step(1, slice_inputs(datas, widths, never.batch_stream_need(1)))
    assert never.batch_stream_checkpoint() == blob, "the checkpoint of a job that takes the spectrum is the checkpoint of one that never did"
    never.close()
    dst = job.configured()                                           # a fresh context, the switch set again
    assert dst.batch_stream_resume(metas, RATE, "lpcm24", blob, **KW) == BLOCK
    outs = dst.batch_stream_step(2, slice_inputs(datas, widths, dst.batch_stream_need(2)))
    got = dst.batch_spectrum()
    dst.batch_stream_close()
    dst.close()
    assert np.concatenate([first, got], axis=1).tobytes() == spec.tobytes()
    for r in range(NCH + 3):
        assert outs[r].tobytes() == raw[r][BLOCK * 3:]


def test_bands_with_a_source_map_and_with_dither(plain):
    job, raw, spec = plain
    pkg = package()
    copied = [job.inputs[0], job.inputs[0]]
    raw_c, spec_c = one_call(job, inputs=copied)
    ctx = job.configured()
    ctx.batch_set_sources([0, 0])                                    # channel 1 reads channel 0's entry
    res = ctx.batch_run([job.inputs[0], None], RATE, "lpcm24", **KW)
    spec_m = ctx.batch_spectrum()
    ctx.close()
    assert spec_m.tobytes() == spec_c.tobytes() and [o.tobytes() for o in res] == raw_c
    assert spec_c[1].tobytes() != spec[1].tobytes()
    ctx = job.configured()
    ctx.batch_set_dither(1, seed=99)
    res = ctx.batch_run(job.inputs, RATE, "lpcm24", **KW)
    spec_d = ctx.batch_spectrum()
    ctx.close()
    assert spec_d.tobytes() == spec.tobytes(), "the bands are taken in front of the dither"
    assert [o.tobytes() for o in res] != raw
    assert pkg.GDG_OK == 0


def test_switches(plain):
    """every run on a fresh context: a second job on a used one starts from the first one's delay lines and metronome position"""
    pkg = package()
    job, raw, spec = plain
    run = lambda c: [o.tobytes() for o in c.batch_run(job.inputs, RATE, "lpcm24", **KW)]
    # off: bytes, device memory and report of a context that never heard of the feature
    never = job.configured(edges=None, report=True)
    assert run(never) == raw, "the spectrum on changes no output byte"
    rep = never.batch_report()
    kib = never.get_option("stat_batch_device_kib")
    with pytest.raises(pkg.GdgError) as e:
        never.batch_spectrum()
    assert e.value.code == pkg.GDG_ERR_INVALID and "no spectrum" in str(e.value)
    never.close()
    off = job.configured(report=True)
    off.batch_spectrum_enable(None)
    assert run(off) == raw
    assert off.batch_report().tobytes() == rep.tobytes() and off.get_option("stat_batch_device_kib") == kib
    with pytest.raises(pkg.GdgError):
        off.batch_spectrum()
    off.close()
    # both together: each of them alone
    both = job.configured(report=True)
    assert run(both) == raw
    assert both.batch_report().tobytes() == rep.tobytes() and both.batch_spectrum().tobytes() == spec.tobytes()
    both.close()
    raw_s, spec_s = streamed(job, (2, 1), 2, report=True)
    assert raw_s == raw and spec_s.tobytes() == spec.tobytes()
    # the spectrum alone (`plain`), a report that was switched off again, and a refused list, which leaves the one in force
    alone = job.configured(report=True)
    alone.batch_report_enable(False)
    bad = np.array([10.0, 5.0])
    assert pkg.lib().gdg_batch_spectrum_enable(alone._h, bad.ctypes.data, 2) == pkg.GDG_ERR_INVALID
    assert run(alone) == raw and alone.batch_spectrum().tobytes() == spec.tobytes()
    with pytest.raises(pkg.GdgError):
        alone.batch_report()
    # too little room says so, with the counts; the counts alone need none
    ports, blocks, bands = C.c_int(0), C.c_size_t(0), C.c_int(0)
    few = np.zeros(5)
    assert pkg.lib().gdg_batch_spectrum(alone._h, few.ctypes.data, few.size, C.byref(ports), C.byref(blocks), C.byref(bands)) == pkg.GDG_ERR_INVALID
    assert (ports.value, blocks.value, bands.value) == (NCH + 3, BLOCKS, len(EDGES) - 1) and "room for 5 values" in pkg.lib().gdg_last_error(alone._h).decode()
    ports, blocks, bands = C.c_int(0), C.c_size_t(0), C.c_int(0)
    assert pkg.lib().gdg_batch_spectrum(alone._h, None, 0, C.byref(ports), C.byref(blocks), C.byref(bands)) == pkg.GDG_OK
    assert (ports.value, blocks.value, bands.value) == (NCH + 3, BLOCKS, len(EDGES) - 1)
    alone.close()
    # while a streamed job is open the switch is refused and nothing changes
    held = job.configured()
    metas, datas, widths = held._stream_split(job.inputs)
    held.batch_stream_open(metas, RATE, "lpcm24", **KW)
    two = np.array([100.0, 200.0])
    assert pkg.lib().gdg_batch_spectrum_enable(held._h, two.ctypes.data, 2) == pkg.GDG_ERR_INVALID
    assert pkg.lib().gdg_batch_spectrum_enable(held._h, None, 0) == pkg.GDG_ERR_INVALID
    outs = held.batch_stream_step(3, slice_inputs(datas, widths, held.batch_stream_need(3)))
    assert held.batch_spectrum().tobytes() == spec.tobytes() and [o.tobytes() for o in outs] == raw
    held.batch_stream_close()
    held.close()
