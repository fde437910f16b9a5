"""The transfer records (include/gdg.h, TRANSFER) on the device: per block and (port, target) pair the auto-spectra and the cross-spectrum in
groups of D bins.  What holds the kernel: the numpy restatement (tests/transfer_ref.py) within 1e-12 of the block's totals at every length at
which the padding takes another path; the header's known answers; silence as +0.0 bytes; a port 2^-30 below its target against its OWN
total; NaN sentinels around everything that may be addressed and the scalar path's bytes against the 16-byte path's; the bits of a pair's
part under everything the definition says it does not depend on; the list checked before anything is launched; and the batch form at 4
channels, 1 blend and 3 blocks + 5 samples: the same bytes whatever the window, the slicing, a checkpoint and resume or a source map, and
those of the stand-alone call on the call's own IEEE64 files."""
import numpy as np
import pytest

import transfer_ref as ref
from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
# The band spectrum's figure and its reasoning (tests/test_gpu_block_spectrum.py): a float64 transform of 8192 points carries a relative error
# of a few 1e-16 x log2(8192) against the block's total power in every bin; the device and numpy order their butterflies differently, so the
# two differ by about twice that; a group adds at most 64 such bins.  1e-12 of the total leaves two orders of magnitude.
TOL = 1e-12


@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    wrong = np.flatnonzero(got.reshape(-1).view(np.uint64) != want.reshape(-1).view(np.uint64))
    assert wrong.size == 0, "%s: %d of %d entries differ, the first at %d: %r, not %r" % (what, wrong.size, got.size, wrong[0], got.reshape(-1)[wrong[0]], want.reshape(-1)[wrong[0]])


def random_rows(n_rows, samples, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (n_rows, samples))
    x *= 10.0 ** rng.uniform(-3, 1, (n_rows, 1))                                 # every row at a level of its own
    return x


def within(got, rows, pairs, D, what):
    want = ref.record(rows, pairs, D)
    T = ref.totals(rows, pairs)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want) / np.where(T > 0.0, T, 1.0)
    worst = float(err.max()) if err.size else 0.0
    print("%s: worst |got - ref| / T = %.3g" % (what, worst))
    assert worst <= TOL, (what, worst, np.unravel_index(int(err.argmax()), err.shape))
    assert not np.signbit(got).any() or np.all(got[np.signbit(got)] != 0.0), "%s: a -0.0 entry" % what


def test_the_symbols_exist():
    pkg = package()
    for name in ("gdg_batch_transfer_enable", "gdg_batch_transfers", "gdg_batch_transfer", "gdg_block_transfer_rows", "gdg_block_transfer_rows_device", "gdg_transfer_doubles",
                 "gdg_match_taps_from_transfer"):
        assert getattr(pkg.lib(), name) is not None and name in pkg.ABI_SYMBOLS
    for name in ("batch_transfer_enable", "batch_transfers", "batch_transfer", "block_transfer", "block_transfer_device", "transfer_doubles", "match_taps_from_transfer"):
        assert callable(getattr(pkg.Context, name))
    assert pkg.transfer_doubles(3, 64) == 3 * 65 * 4 == ref.doubles(3, 64)


# ---- 7. against the numpy restatement ------------------------------------------------------------------------------------------------------
PAIRS16 = [(0, 1), (1, 0), (2, 2), (0, 2), (0, 1), (3, 0), (1, 3), (2, 1), (3, 3), (0, 3), (1, 1), (2, 0), (3, 2), (1, 2), (0, 0), (3, 1)]


@pytest.mark.parametrize("samples", [1, 2, 8191, 8192, 8193, 8192 + 5])
def test_against_the_numpy_restatement_at_every_length(ctx1, samples):
    x = random_rows(4, samples, samples)
    for D, pairs in ((1, [(0, 1)]), (2, [(1, 1), (0, 2)]), (64, PAIRS16)):          # 1, 2 and 16 pairs; port == target; a port that repeats
        within(ctx1.block_transfer(x, pairs, D), x, pairs, D, "samples %d, D %d, %d pairs" % (samples, D, len(pairs)))


@pytest.mark.parametrize("D", [1, 2, 64])
def test_against_the_numpy_restatement_at_every_pair_count(ctx1, D):
    x = random_rows(4, BLOCK + 5, 70 + D)
    for pairs in ([(2, 3)], [(3, 3), (1, 0)], PAIRS16):
        within(ctx1.block_transfer(x, pairs, D), x, pairs, D, "D %d, %d pairs" % (D, len(pairs)))


# ---- 8. the header's known answers ------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_header(ctx1):
    n = np.arange(BLOCK)
    x = np.stack([0.5 * np.cos(2.0 * np.pi * 100.0 * n / BLOCK), 0.5 * np.sin(2.0 * np.pi * 100.0 * n / BLOCK)])
    T = ref.totals(x, [(0, 1)])[0, 0, 0]
    assert abs(T[0] - 0.25 / 4) <= 1e-15 and abs(T[1] - 0.25 / 4) <= 1e-15
    got = ctx1.block_transfer(x, [(0, 1)], 1)[0, 0]
    for g, sxx in ((99, 0.25 / 24), (100, 0.25 / 6), (101, 0.25 / 24)):
        assert abs(got[g, 0] - sxx) <= TOL * T[0] and abs(got[g, 1] - sxx) <= TOL * T[1], (g, got[g])
        assert abs(got[g, 2]) <= TOL * T[2] and abs(got[g, 3] + sxx) <= TOL * T[3], (g, got[g])
    others = np.delete(got, [99, 100, 101], axis=0)
    assert np.abs(others).max() <= TOL * T[0]
    # D = 4: group g holds the bins 4 g - 1 .. 4 g + 2, so 99, 100 and 101 (and the empty 102) lie in group 25
    assert [ref.group_bins(25, 4), ref.group_bins(24, 4), ref.group_bins(26, 4)] == [(99, 102), (95, 98), (103, 106)]
    got = ctx1.block_transfer(x, [(0, 1)], 4)[0, 0]
    assert abs(got[25, 0] - 0.25 / 4) <= TOL * T[0] and abs(got[25, 1] - 0.25 / 4) <= TOL * T[1] and abs(got[25, 2]) <= TOL * T[2] and abs(got[25, 3] + 0.25 / 4) <= TOL * T[3]
    assert np.abs(np.delete(got, 25, axis=0)).max() <= TOL * T[0]


def test_parseval_in_the_raw_form(ctx1):
    x = random_rows(1, BLOCK, 5)
    wx = ref.window() * x[0]
    X = np.fft.fft(wx)
    want = (BLOCK * np.sum(wx * wx) + abs(X[0]) ** 2 + abs(X[BLOCK // 2]) ** 2) / (2.0 * ref.SCALE)
    for D in (1, 8):
        got = ctx1.block_transfer(x, [(0, 0)], D)[0, 0]
        assert abs(got[:, 0].sum() - want) <= TOL * want and abs(got[:, 2].sum() - want) <= TOL * want, (D, got[:, 0].sum(), want)
        # port == target: x rides in both parts of the one transform, whose two outputs round on their own -- equal to the tolerance, not to the bit
        assert np.abs(got[:, 0] - got[:, 1]).max() <= TOL * want and np.abs(got[:, 0] - got[:, 2]).max() <= TOL * want and np.abs(got[:, 3]).max() <= TOL * want


# ---- 9. silence ---------------------------------------------------------------------------------------------------------------------------------
def test_a_silent_side_is_plus_zero_as_bytes(ctx1):
    x = random_rows(3, 2 * BLOCK, 9)
    x[1] = 0.0                                                                   # a silent row
    x[2, :BLOCK] = np.nan                                                        # an all-NaN block ...
    x[2, 3] = np.inf
    x[0, BLOCK:] = -0.0                                                          # ... and a block of -0.0
    for D in (1, 16):
        got = ctx1.block_transfer(x, [(1, 0), (0, 1), (2, 0), (0, 2), (1, 1)], D)
        zero = lambda a, what: same(a, np.zeros_like(a), "D %d: %s" % (D, what))
        zero(got[:, 0, :, [0, 2, 3]], "a silent port")
        zero(got[:, 1, :, [1, 2, 3]], "a silent target")
        zero(got[0, 2, :, [0, 2, 3]], "an all-NaN port block")
        zero(got[0, 3, :, [1, 2, 3]], "an all-NaN target block")
        zero(got[1, 2, :, [1, 2, 3]], "a target block of -0.0")
        zero(got[:, 4], "silence against itself")
        assert got[0, 0, :, 1].all() and got[0, 1, :, 0].all()                   # the side that sounds is there
    within(ctx1.block_transfer(x, [(1, 0), (2, 0), (0, 2)], 1), x, [(1, 0), (2, 0), (0, 2)], 1, "beside silence")


# ---- 10. levels ---------------------------------------------------------------------------------------------------------------------------------
def test_a_port_far_below_its_target_keeps_its_own_spectrum(ctx1):
    rng = np.random.default_rng(10)
    x = np.stack([rng.uniform(-1, 1, BLOCK + 5) * 2.0 ** -30, rng.uniform(-1, 1, BLOCK + 5)])
    for D in (1, 64):
        within(ctx1.block_transfer(x, [(0, 1)], D), x, [(0, 1)], D, "2^-30, D %d" % D)         # Sxx against sum Pxx of the port itself


# ---- 11. nothing outside the rows and the records; the two load paths --------------------------------------------------------------------------
def test_nan_sentinels_and_the_scalar_path_gives_the_vector_path_s_bytes(ctx1):
    pkg = package()
    samples, n_rows, D, pairs = BLOCK + 5, 3, 2, [(0, 2), (1, 1)]
    x = random_rows(n_rows, samples, 11)
    want = ctx1.block_transfer(x, pairs, D)
    n = 2 * pkg.transfer_doubles(len(pairs), D)                                  # two blocks

    def run(host, row0, stride, rec_words, rec0, what):
        d_rows, d_rec = ctx1.alloc(1, host.size), ctx1.alloc(1, rec_words)
        assert d_rows.ptr % 16 == 0 and d_rec.ptr % 16 == 0
        d_rows.upload(host)
        d_rec.upload(np.full(rec_words, np.nan))
        ctx1.block_transfer_device(d_rows.ptr + 8 * row0, stride, n_rows, samples, pairs, D, d_rec.ptr + 8 * rec0)
        out, back = d_rec.download().reshape(-1), d_rows.download().reshape(-1)
        d_rows.free()
        d_rec.free()
        assert np.isnan(out[:rec0]).all() and np.isnan(out[rec0 + n:]).all(), "%s: the sentinels around the records" % what
        same(out[rec0:rec0 + n].reshape(want.shape), want, what)
        assert np.array_equal(back, host, equal_nan=True)

    stride = samples + (samples & 1) + 2                                         # even: `lead` decides the alignment of every row
    for lead, what in ((2, "rows at 16 bytes (VEC)"), (1, "rows at an odd 8-byte offset (scalar)")):
        host = np.full(lead + n_rows * stride + 8, np.nan)
        for r in range(n_rows):
            host[lead + r * stride:lead + r * stride + samples] = x[r]
        run(host, lead, stride, 2 + n + 2, 2, what)
    # rows of an odd stride, and records at an odd 8-byte offset: the four 8-byte stores give the bytes of the two 16-byte ones
    run(np.ascontiguousarray(x).reshape(-1), 0, samples, 1 + n + 3, 1, "records at an odd offset")


# ---- 12. the bits of a pair's part ----------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_place_neighbours_rows_or_row_count(ctx1):
    samples = BLOCK + 5
    x = random_rows(6, samples, 12)
    for D in (1, 8):
        alone = ctx1.block_transfer(x[[2, 4]], [(0, 1)], D)[:, 0]
        for rows, pairs, at in ((x, [(2, 4)], 0), (x, [(0, 1), (2, 4)], 1), (x, PAIRS16[:15] + [(2, 4)], 15), (x[[4, 5, 2]], [(1, 1), (2, 0), (0, 2)], 1),
                                (x[::-1], [(3, 1), (5, 5)], 0)):
            same(ctx1.block_transfer(rows, pairs, D)[:, at], alone, "D %d, %d rows, pair %d of %d" % (D, len(rows), at, len(pairs)))


# ---- 13. the list is checked before anything is launched ------------------------------------------------------------------------------------------
def test_a_list_is_checked_before_anything_is_launched(ctx1):
    pkg = package()
    words = pkg.transfer_doubles(16, 1) + 4
    d_rows, d_rec = ctx1.alloc(1, 3 * 64), ctx1.alloc(1, words)
    d_rows.upload(random_rows(3, 64, 13).reshape(-1))
    d_rec.upload(np.full(words, np.nan))
    for pairs, D, what in (([(0, 1), (3, 1)], 1, "pair 1 names row 3 of 3"), ([(0, 1), (1, 3)], 1, "pair 1 has the target row 3 of 3"), ([(0, 1)] * 17, 1, "17 pairs; 0 \\(off\\) to 16"),
                           ([(0, 1)], 0, "a group width of 0 bins"), ([(0, 1)], 128, "a group width of 128 bins"), ([(0, 1)], 3, "a group width of 3 bins"), ([(-1, 1)], 1, "pair 0 names row -1")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx1.block_transfer_device(d_rows.ptr, 64, 3, 64, pairs, D, d_rec.ptr)
        assert e.value.code == pkg.GDG_ERR_INVALID
    out = d_rec.download().reshape(-1)
    d_rows.free()
    d_rec.free()
    assert np.isnan(out).all(), "the record buffer keeps its sentinel"


# ---- 14, 15. the batch form ------------------------------------------------------------------------------------------------------------------------
RATE, NCH = 48000, 4
SAMPLES = 3 * BLOCK + 5
BLOCKS = 4
NO = NCH + 3
BLENDS = [[(0, 0.6), (1, -0.3)]]                                                # port NO
PAIRS = [(0, 1), (2, NO), (NCH, 3), (1, 1)]                                     # a blend port as a target; master left as a port; port == target
GROUP = 32
FITS = [(0, [1])]
GRAM = [0, 1, 2]
TAPFITS = [(1, [0], 4)]


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """4 channels on one source with power amps of different random taps"""

    def __init__(self):
        self.pkg = package()
        self.file = lpcm16_file(0.1 * synth_signal(0, SAMPLES, RATE) + 0.2 * np.random.default_rng(14).uniform(-1.0, 1.0, SAMPLES))
        self.inputs = [(self.file, "lpcm16", RATE)] + [None] * (NCH - 1)
        self.metas = [(SAMPLES, "lpcm16", RATE)] + [None] * (NCH - 1)
        self.irs = [synth_ir(n, seed=740 + c) for c, n in enumerate((300, 64, 128, 12))]
        self.cache = {}

    def configured(self, window=2, pairs=PAIRS, group=GROUP, source_map=True, never=False, others=False):
        ctx = self.pkg.Context(NCH, BLOCK)
        for c in range(NCH):
            ctx.append_unit(c, "power_amp", fir=self.irs[c])
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(NCH):
            ctx.spatializer_set_position(c, -60.0 + 30.0 * c, 1.0 + 0.25 * c, 0.8)
        ctx.set_window(window)
        if source_map:
            ctx.batch_set_sources([0] * NCH)
        ctx.batch_set_blends(BLENDS)
        ctx.batch_report_enable(True)
        if others:
            ctx.batch_fit_enable(FITS)
            ctx.batch_gram_enable(GRAM)
            ctx.batch_tapfit_enable(TAPFITS)
        if not never:
            ctx.batch_transfer_enable(pairs, group)
        return ctx

    def run(self, window=2, pairs=PAIRS, group=GROUP, never=False, others=False):
        key = (window, str(pairs), group, never, others)
        if key not in self.cache:
            ctx = self.configured(window, pairs, group, never=never, others=others)
            outs = ctx.batch_run(self.inputs, RATE, "ieee64")
            got = dict(outs=outs, transfer=ctx.batch_transfer() if pairs and not never else None, report=ctx.batch_report(), kib=ctx.get_option("stat_batch_device_kib"))
            if others:
                got.update(fit=ctx.batch_fit(), gram=ctx.batch_gram(), tapfit=ctx.batch_tapfit())
            self.cache[key] = got
            ctx.close()
        return self.cache[key]


@pytest.fixture(scope="module")
def job():
    return Job()


def test_batch_records_are_those_of_the_stand_alone_call_on_the_call_s_own_files(job, ctx1):
    run = job.run()
    rows = np.stack([o.view(np.float64) for o in run["outs"]])
    assert rows.shape == (NO + 1, BLOCKS * BLOCK) and np.isfinite(rows).all() and all(r.any() for r in rows[:NCH])
    assert run["transfer"].shape == (BLOCKS, ref.doubles(len(PAIRS), GROUP)) and run["transfer"].any()
    alone = ctx1.block_transfer(rows, PAIRS, GROUP)
    same(run["transfer"], alone.reshape(BLOCKS, -1), "batch against stand-alone")
    within(alone, rows, PAIRS, GROUP, "the call's own files")


def test_batch_records_are_the_same_bytes_however_the_job_is_cut(job):
    want = job.run(window=1)["transfer"]
    same(job.run(window=2)["transfer"], want, "window 2 against window 1")
    same(job.run(window=16)["transfer"], want, "window 16 against window 1")
    for cuts in ((1, 2, 1), (2, 1, 1)):
        ctx = job.configured()
        parts, todo = [], list(cuts)
        for _ in ctx.batch_stream(job.inputs, RATE, "ieee64", lambda left: todo.pop(0)):
            parts.append(ctx.batch_transfer())
        ctx.close()
        assert [p.shape[0] for p in parts] == list(cuts)
        same(np.concatenate(parts, axis=0), want, "slices of %d + %d + %d" % cuts)


def test_checkpoint_resume_and_no_source_map_give_the_same_records(job):
    """the one file named four times instead of through a source map (a reader refuses the checkpoint calls), cut after the first block,
    resumed in a fresh context on which the list is set again: the list is configuration, and the record is stateless"""
    want = job.run()["transfer"]
    metas = [job.metas[0]] * NCH
    cut = lambda need: [job.file[2 * f:2 * (f + c)] for f, c in need]
    ctx = job.configured(source_map=False)
    assert ctx.batch_stream_open(metas, RATE, "ieee64") == BLOCKS * BLOCK
    ctx.batch_stream_step(1, cut(ctx.batch_stream_need(1)))
    head = ctx.batch_transfer()
    blob = ctx.batch_stream_checkpoint()
    ctx.batch_stream_close()
    ctx.close()
    ctx = job.configured(source_map=False)
    assert ctx.batch_stream_resume(metas, RATE, "ieee64", blob) == BLOCK
    ctx.batch_stream_step(3, cut(ctx.batch_stream_need(3)))
    tail = ctx.batch_transfer()
    ctx.batch_stream_close()
    ctx.close()
    same(np.concatenate([head, tail], axis=0), want, "checkpoint and resume, no source map")


def test_a_list_changes_no_output_byte_no_other_record_and_is_counted_and_off_is_never(job):
    on, never, off = job.run(others=True), job.run(never=True, others=True), job.run(pairs=[], others=True)
    for r in range(NO + 1):
        assert np.array_equal(on["outs"][r], never["outs"][r]) and np.array_equal(off["outs"][r], never["outs"][r]), r
    for kind in ("report", "fit", "gram", "tapfit"):
        assert on[kind].tobytes() == never[kind].tobytes() == off[kind].tobytes(), kind
    same(on["transfer"], job.run()["transfer"], "beside the three lists")
    assert off["kib"] == never["kib"]
    # the table (two ints per pair and the width) and the room in each of the two download halves (16 + window x doubles): the option counts whole KiB
    grown = 4 * (2 * len(PAIRS) + 1) + 2 * (16 + 2 * ref.doubles(len(PAIRS), GROUP) * 8)
    assert grown // 1024 <= on["kib"] - never["kib"] <= -(-grown // 1024), (on["kib"], never["kib"], grown)
    ctx = job.configured()
    assert ctx.batch_transfers() == len(PAIRS)
    ctx.batch_run(job.inputs, RATE, "ieee64")
    ctx.batch_transfer_enable([])                                                # off after having been on
    assert ctx.batch_transfers() == 0
    outs = ctx.batch_run(job.inputs, RATE, "ieee64")
    with pytest.raises(job.pkg.GdgError, match="ran without them"):
        ctx.batch_transfer()
    kib = ctx.get_option("stat_batch_device_kib")
    ctx.close()
    fresh = job.configured(never=True)
    fresh.batch_run(job.inputs, RATE, "ieee64")
    want_outs = fresh.batch_run(job.inputs, RATE, "ieee64")                      # the second job of a context, as above
    assert kib == fresh.get_option("stat_batch_device_kib")
    fresh.close()
    for r in range(NO + 1):
        assert np.array_equal(outs[r], want_outs[r]), r


def test_refusals(job):
    pkg = job.pkg
    ctx = job.configured(never=True)
    with pytest.raises(pkg.GdgError, match="no transfer records") as e:          # before any call
        ctx.batch_transfer()
    assert e.value.code == pkg.GDG_ERR_INVALID
    for pairs, D, what in (([(0, 1)], 3, "a group width of 3 bins"), ([(0, 1), (-1, 0)], 1, "pair 1 names port -1"), ([(0, -2)], 1, "pair 0 has the target port -2"),
                           ([(0, 1)] * 17, 1, "17 pairs")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx.batch_transfer_enable(pairs, D)
        assert e.value.code == pkg.GDG_ERR_INVALID and ctx.batch_transfers() == 0
    # a port at N + 3 + B: taken as configuration, refused and named when the job is described
    ctx.batch_transfer_enable([(0, 1), (NO + 1, 0)], 1)
    with pytest.raises(pkg.GdgError, match="pair 1 has the measured port %d" % (NO + 1)) as e:
        ctx.batch_run(job.inputs, RATE, "ieee64")
    assert e.value.code == pkg.GDG_ERR_INVALID
    ctx.batch_transfer_enable([(0, NO + 1)], 1)
    with pytest.raises(pkg.GdgError, match="pair 0 has the target port %d" % (NO + 1)):
        ctx.batch_stream_open(job.metas, RATE, "ieee64")
    with pytest.raises(pkg.GdgError, match="no transfer records"):
        ctx.batch_transfer()
    # enabling while a streamed job is open: refused, and the list in force stays
    ctx.batch_transfer_enable([(0, 1)], 4)
    ctx.batch_stream_open(job.metas, RATE, "ieee64")
    with pytest.raises(pkg.GdgError, match="a streamed batch run is open") as e:
        ctx.batch_transfer_enable([(0, 2)], 8)
    assert e.value.code == pkg.GDG_ERR_INVALID and ctx.batch_transfers() == 1
    ctx.batch_stream_close()
    ctx.close()
    # the shard calls, with a list in force (and no blends, which they refuse first)
    ctx = job.configured(pairs=[(0, 1)])
    ctx.batch_set_blends([])
    for call, args in ((ctx.batch_run_shard, (job.inputs, RATE, "ieee64")), (ctx.batch_stream_open_shard, (job.metas, RATE, "ieee64"))):
        with pytest.raises(pkg.GdgError, match="1 transfer pairs are in force") as e:
            call(*args)
        assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    ctx.close()
    # ... and the other two: a shard's job opened and cut without a list, the list enabled once it is closed -- a step and a resume refuse
    ctx = job.configured(never=True, source_map=False)
    ctx.batch_set_blends([])
    metas = [job.metas[0]] * NCH
    ctx.batch_stream_open_shard(metas, RATE, "ieee64")
    blob = ctx.batch_stream_checkpoint()
    ctx.batch_stream_close()
    ctx.batch_transfer_enable([(0, 1)], 2)
    with pytest.raises(pkg.GdgError, match="gdg_batch_stream_resume_shard: 1 transfer pairs are in force") as e:
        ctx.batch_stream_resume_shard(metas, RATE, "ieee64", blob)
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    with pytest.raises(pkg.GdgError, match="gdg_batch_stream_step_shard: 1 transfer pairs are in force") as e:
        ctx.batch_stream_step_shard(1, [None] * NCH)
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    ctx.close()


# ---- 16. end to end: records -> planner -> taps on an amp ------------------------------------------------------------------------------------------
E_BLOCKS, E_TAPS, E_IR, E_GROUP = 16, 16, 12, 32
PLAN_TOL = 4 * 6.6e-15                                                          # tests/test_transfer_host.py: the C planner against irfft, margin 4


def e2e_take():
    x = np.random.default_rng(16).standard_normal(E_BLOCKS * BLOCK)
    return np.round(0.25 * x / 4.0 * 32767.0).clip(-32767, 32767) / 32767.0


def e2e_ir():
    return np.random.default_rng(116).uniform(-1.0, 1.0, E_IR)


def tap_distance(taps, ir):
    """the planned taps with the taper taken off against the true response padded with zeros, as a share of its largest tap"""
    true = np.zeros(E_TAPS)
    true[:E_IR] = ir
    return float(np.max(np.abs(taps / ref.taper(E_TAPS, 0) - true)) / np.max(np.abs(ir)))


def test_end_to_end_planned_taps_match_the_restatement_and_close_the_gap(ctx1):
    """Two channels read one noise take of 16 blocks; channel 0 ends in a power amp set to a unit impulse, channel 1 in one with a random
    12-tap response.  Pass 1 keeps the transfer records of the pair (0, 1) at D = 32 and the fit record of target 1 against term 0.

    TOLERANCE of the planned taps against transfer_ref.plan on the call's own files.  Test 7 bounds every entry of a block's record by
    1e-12 T of that block; summed over the blocks, |dSxy[g]| <= 1e-12 sum_b Txy =: exy and |dSxx[g]| <= 1e-12 sum_b Txx =: exx.  With
    H = Sxy / Sxx:  |dH[g]| <= (exy + |H[g]| exx) / Sxx[g]  to first order.  A tap is t[m] <= 1 times a mean of H[g] exp(..) over the N'
    bins, so |dtap| <= max_g |dH[g]|.  To that comes test 1's figure for the C planner's transform against irfft, PLAN_TOL max|h|.

    Pass 2 puts the taps on channel 0's amp and runs the job again from the saved state: the fit's residual at its planned weight is
    smaller than in pass 1.  The distance of the taps from the true 12 is compared with the same distance of the numpy restatement on
    CPU-made rows (numpy's convolution), margin 4 -- the estimate's own bias (Hann leakage, 32-bin groups) is in both.  Measured on an
    MI355X: see DESIGN.md 4.12h."""
    pkg = package()
    take, ir = e2e_take(), e2e_ir()
    unit = np.zeros(E_TAPS)
    unit[0] = 1.0
    file = np.ascontiguousarray(np.round(take * 32767.0).astype("<i2")).view(np.uint8)
    inputs = [(file, "lpcm16", RATE), None]
    ctx = pkg.Context(2, BLOCK)
    amp0 = ctx.append_unit(0, "power_amp", fir=unit)
    ctx.append_unit(1, "power_amp", fir=ir)
    ctx.spatializer_set_sample_rate(RATE)
    ctx.set_window(4)
    ctx.batch_set_sources([0, 0])
    ctx.batch_fit_enable([(1, [0])])
    ctx.batch_transfer_enable([(0, 1)], E_GROUP)
    blob = ctx.save_state()
    outs = ctx.batch_run(inputs, RATE, "ieee64")
    rows = np.stack([o.view(np.float64) for o in outs])[:2]
    rec = ctx.batch_transfer()
    _, res1 = pkg.blend_weights_from_fit(ctx.batch_fit())
    taps, coh = pkg.match_taps_from_transfer(rec, 1, E_GROUP, E_TAPS, 0)
    want_rec = ref.record(rows, [(0, 1)], E_GROUP)
    want, want_coh = ref.plan(want_rec, 1, E_GROUP, E_TAPS, 0)
    T = ref.totals(rows, [(0, 1)]).sum(axis=0)[0, 0]                            # sum over the blocks of Txx, Tyy, Txy, Txy
    s = want_rec.sum(axis=0)[0]
    Hmag = np.hypot(s[:, 2], s[:, 3]) / s[:, 0]
    tol = float(np.max((TOL * T[2] + Hmag * TOL * T[0]) / s[:, 0])) + PLAN_TOL * float(np.max(np.abs(want)))
    err = float(np.max(np.abs(taps[0] - want[0])))
    print("end to end: max |tap - ref| = %.3g (tolerance %.3g), coherence %.6f against %.6f" % (err, tol, coh[0], want_coh[0]))
    assert err <= tol, (err, tol)
    assert abs(coh[0] - want_coh[0]) <= tol and 0.9 < coh[0] <= 1.0 + tol
    # the distance from the truth, beside the restatement's on rows made on the CPU
    cpu_rows = np.stack([take, np.convolve(take, ir)[:take.size]])
    cpu_taps, _ = ref.plan(ref.record(cpu_rows, [(0, 1)], E_GROUP), 1, E_GROUP, E_TAPS, 0)
    d_dev, d_cpu = tap_distance(taps[0], ir), tap_distance(cpu_taps[0], ir)
    print("end to end: distance from the true taps %.4g on the device, %.4g by the restatement on CPU-made rows" % (d_dev, d_cpu))
    assert d_dev <= 4.0 * d_cpu, (d_dev, d_cpu)
    # pass 2: the taps on channel 0's amp, the job again from the saved state
    ctx.unit_set_fir(amp0, taps[0])
    ctx.load_state(blob)
    ctx.batch_run(inputs, RATE, "ieee64")
    _, res2 = pkg.blend_weights_from_fit(ctx.batch_fit())
    print("end to end: residual of target 1 against term 0: %.4g before, %.4g with the planned taps" % (res1[0], res2[0]))
    ctx.close()
    assert res2[0] < res1[0], (res1[0], res2[0])
