"""The tap fit (include/gdg.h, TAPFIT) on the device.  The record kernel slides the lags of a row over LDS and sums on the FP64 matrix
instruction; what holds it: the Gram record of the same rows at T = 1 and of the host-shifted rows at any T, bit for bit (the header's two
consequences); rows of small integers against the int64 Gram at every block length at which the kernel takes another path; random rows
within (L - T + 1) * 2^-52 * sum |a b| of math.fsum; NaN sentinels around everything that may be addressed; the bits of an entry under
everything the definition says it does not depend on; and the batch form at 3 channels, 1 blend and 3 blocks: the same bytes whatever the
window, the slicing, a checkpoint and resume or a source map, and those of the stand-alone call on the call's own IEEE64 files."""
import numpy as np
import pytest

import tapfit_ref as ref
from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
EPS = 2.0 ** -52


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
    x = rng.uniform(-1.5, 1.5, (n_rows, samples))
    x[:, ::7] *= 1e-9
    return x


def integer_rows(n_rows, samples, seed):
    """integers in [-8, 8]: a product is at most 64 and a sum of 8192 of them below 2^20 -- every partial sum is exact in any order"""
    return np.random.default_rng(seed).integers(-8, 9, (n_rows, samples), dtype=np.int64)


def test_the_symbols_exist():
    pkg = package()
    for name in ("gdg_batch_tapfit_enable", "gdg_batch_tapfits", "gdg_batch_tapfit", "gdg_block_tapfit_rows", "gdg_block_tapfit_rows_device", "gdg_tapfit_doubles",
                 "gdg_blend_taps_from_tapfit"):
        assert getattr(pkg.lib(), name) is not None and name in pkg.ABI_SYMBOLS
    for name in ("batch_tapfit_enable", "batch_tapfits", "batch_tapfit", "block_tapfit", "block_tapfit_device"):
        assert callable(getattr(pkg.Context, name))
    assert pkg.tapfit_doubles([(0, [1], 64), (0, [1, 2], 3)]) == 65 * 66 // 2 + 7 * 8 // 2


# ---- 1. the header's two consequences ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 4])
def test_one_tap_and_different_ports_is_the_gram_record_of_the_list(ctx1, K):
    for block, samples in ((8192, 8192 + 5), (100, 250), (3, 7)):
        x = random_rows(K + 2, samples, 10 * K + block)
        ports = [int(p) for p in np.random.default_rng(K).permutation(K + 2)]
        t, terms = ports[0], ports[1:K + 1]
        got = ctx1.block_tapfit(x, [(t, terms, 1)], block)
        same(got, ctx1.block_gram(x, terms + [t], block), "T = 1, K = %d, block %d of %d" % (K, block, samples))


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("T", [2, 3, 4, 5, 16, 17, 63, 64])
def test_one_block_is_the_gram_record_of_the_host_shifted_rows(ctx1, T, K):
    L = 300                                                                      # three chunks of positions at T <= 44, a ragged last group of four
    x = random_rows(K + 1, L, 100 * T + K)
    v = ref.shifted_rows(x, K, list(range(K)), T)
    assert v.shape == (K * T + 1, L - T + 1)
    got = ctx1.block_tapfit(x, [(K, list(range(K)), T)], L)
    same(got, ctx1.block_gram(v, list(range(K * T + 1)), L - T + 1), "T = %d, K = %d" % (T, K))


# ---- 2. exact: integer rows at every block length at which the kernel takes another path ---------------------------------------------------------
def lengths_of(T, chunk):
    """L = T - 1 (no position), T, T + 3, T + 4, T + 5 (one group of four and its borders); block lengths and position counts at the chunk"""
    out = [T - 1, T, T + 3, T + 4, T + 5, chunk - 1, chunk, chunk + 1, chunk + T - 2, chunk + T - 1, chunk + T, 2 * chunk + T]
    return sorted({L for L in out if L >= 1})


@pytest.mark.parametrize("T", [1, 2, 5, 33, 64])
def test_integer_rows_give_the_int64_gram_bit_for_bit(ctx1, T):
    pkg = package()
    fits = [(2, [0], T), (0, [1, 2], T), (1, [1, 0], min(T, 3))]                # one term; two; the target among the terms of another
    for L in lengths_of(T, pkg.TAPFIT_CHUNK):
        xi = integer_rows(3, L, 1000 * T + L)
        got = ctx1.block_tapfit(xi.astype(np.float64), fits, L)
        want = ref.record_int(xi, fits, L)
        assert got.shape == (1, ref.list_doubles(fits))
        same(got, want, "T = %d, L = %d" % (T, L))
        if L < T:
            zero = got[0, :ref.fit_doubles(1, T) + ref.fit_doubles(2, T)]
            assert not zero.any() and not np.signbit(zero).any(), "L < T: every entry is +0.0"


@pytest.mark.parametrize("block,samples", [(8192, 8192 + 5), (100, 250)])
def test_integer_rows_over_several_blocks_and_a_short_last_one(ctx1, block, samples):
    fits = [(0, [1, 2], 64), (2, [0, 1, 1, 0], 7), (1, [2], 17)]                 # 129 virtual rows: three tile rows; a port twice
    xi = integer_rows(3, samples, block)
    got = ctx1.block_tapfit(xi.astype(np.float64), fits, block)
    same(got, ref.record_int(xi, fits, block), "block %d of %d" % (block, samples))


# ---- 3. the error bound ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,samples,T,K", [(8192, 8192 + 5, 64, 2), (100, 250, 17, 1), (8192, 8192, 5, 4)])
def test_random_rows_lie_within_the_bound_of_fsum(ctx1, block, samples, T, K):
    """every checked entry within (L - T + 1) * 2^-52 * sum |a b| of math.fsum: it holds for any order of that many fused or unfused terms.
    Checked: 150 entries drawn once, the target's whole row, and the corners of the record."""
    x = random_rows(K + 1, samples, 7 * T + K)
    got = ctx1.block_tapfit(x, [(K, list(range(K)), T)], block)
    V = K * T + 1
    ii, jj = np.tril_indices(V)
    pick = np.unique(np.concatenate([np.random.default_rng(T).choice(ii.size, min(150, ii.size), replace=False), np.flatnonzero(ii == V - 1), [0, ii.size - 1]])).astype(int)
    for b in range(-(-samples // block)):
        L = min(block, samples - b * block)
        v = ref.shifted_rows(x, K, list(range(K)), T, b * block, L)
        for e in pick:
            exact, mag = ref.entry_fsum(v, ii[e], jj[e])
            assert abs(got[b, e] - exact) <= max(L - T + 1, 0) * EPS * mag, (b, int(ii[e]), int(jj[e]), got[b, e], exact)


# ---- 4. padding --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,samples,fits", [(8192, 8192 + 5, [(2, [0, 1], 64)]), (100, 250, [(0, [1], 17), (1, [2, 0], 3)]), (6, 15, [(1, [0], 4)])])
def test_nan_sentinels_around_the_addressed_range_change_nothing(ctx1, block, samples, fits):
    """rows at an odd offset with a stride of samples + 3: NaN directly in front of the first row, between the rows, behind the last one, a
    whole NaN row that no fit names, and a guard word behind the records -- one sample read outside [row, row + samples), and entries turn
    NaN; one double written behind the records, and the guard is gone"""
    x = random_rows(3, samples, samples)
    want = ctx1.block_tapfit(x, fits, block)
    assert np.isfinite(want).all()
    stride, off = samples + 3, 1
    padded = np.full(off + 4 * stride + 2, np.nan)
    for r in range(3):
        padded[off + r * stride:off + r * stride + samples] = x[r]
    d_rows, d_rec = ctx1.alloc(1, padded.size), ctx1.alloc(1, want.size + 1)
    d_rows.upload(padded)
    d_rec.upload(np.full(want.size + 1, 7.0))
    ctx1.block_tapfit_device(d_rows.ptr + 8 * off, stride, 4, samples, fits, d_rec.ptr, block)
    raw = d_rec.download().reshape(-1)
    d_rows.free()
    d_rec.free()
    assert raw[want.size] == 7.0, "the guard word behind the last record was written"
    same(raw[:want.size].reshape(want.shape), want, "strided rows between NaN")


# ---- 5. the order, as defined ------------------------------------------------------------------------------------------------------------------
def test_an_entry_s_bits_do_not_depend_on_k_the_position_or_the_other_fits(ctx1):
    """port p against target t at T = 17: alone; as the second term of a two-term fit behind another fit; as the third of four terms at
    the end of a list -- the entries among p's lags and the target are the same bits"""
    T, samples = 17, BLOCK + 5
    x = random_rows(5, samples, 99)
    p, t = 3, 1
    alone = ctx1.block_tapfit(x, [(t, [p], T)], BLOCK)
    V1 = T + 1
    ii, jj = np.tril_indices(V1)

    def part(rec, fits, f, j):
        """of fit f, the entries among term j's lags and the target, in the layout of a one-term record"""
        off = sum(ref.fit_doubles(len(ports), taps) for _, ports, taps in fits[:f])
        K = len(fits[f][1])
        where = lambda u: K * T if u == T else j * T + u
        idx = [off + max(where(a), where(b)) * (max(where(a), where(b)) + 1) // 2 + min(where(a), where(b)) for a, b in zip(ii, jj)]
        return rec[:, idx]

    for fits, f, j in (([(0, [2], 5), (t, [0, p], T)], 1, 1), ([(t, [4, 0, p, 2], T)], 0, 2), ([(t, [p, p], T), (2, [0], 64), (t, [2, p], T)], 2, 1)):
        same(part(ctx1.block_tapfit(x, fits, BLOCK), fits, f, j), alone, str(fits))


def test_a_list_is_checked_before_anything_is_launched(ctx1):
    pkg = package()
    x = random_rows(3, 64, 1)
    for fits, what in (([(0, [3], 2)], "fit 0, term 0 names row 3 of 3"), ([(0, [1], 2), (3, [1], 2)], "fit 1 has the target row 3 of 3"), ([(0, [1], 0)], "fit 0 has 0 taps per term; 1 to 64"),
                       ([(0, [1], 65)], "fit 0 has 65 taps per term"), ([(0, [1, 2, 0], 64)], "fit 0 has 3 terms x 64 taps = 192 unknowns; at most 128"),
                       ([(0, [1, 2, 0, 1, 2], 2)], "fit 0 has 5 terms; 1 to 4"), ([(0, [], 2)], "fit 0 has 0 terms"), ([(0, [1], 2)] * 17, "17 fits; 0 \\(off\\) to 16")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx1.block_tapfit(x, fits)
        assert e.value.code == pkg.GDG_ERR_INVALID
    with pytest.raises(pkg.GdgError, match="blocks of 0 samples"):
        ctx1.block_tapfit(x, [(0, [1], 2)], 0)


# ---- 6. the batch form -------------------------------------------------------------------------------------------------------------------------
RATE, NCH, BLOCKS = 48000, 3, 3
SAMPLES = 2 * BLOCK + 1000
NO = NCH + 3
BLENDS = [[(0, 0.6), (1, -0.3)]]                                                # port NO
FITS = [(NO, [0, 1], 16), (NCH, [2], 64), (0, [NO], 1)]                         # a blend port as a target and as a term; master left


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """3 channels on one source with power amps of different random taps"""

    def __init__(self):
        self.pkg = package()
        self.file = lpcm16_file(0.1 * synth_signal(0, SAMPLES, RATE) + 0.2 * np.random.default_rng(11).uniform(-1.0, 1.0, SAMPLES))
        self.inputs = [(self.file, "lpcm16", RATE)] + [None] * (NCH - 1)
        self.metas = [(SAMPLES, "lpcm16", RATE)] + [None] * (NCH - 1)
        self.irs = [synth_ir(n, seed=730 + c) for c, n in enumerate((300, 64, 128))]
        self.cache = {}

    def configured(self, window=2, fits=FITS, source_map=True, never=False):
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
        if not never:
            ctx.batch_tapfit_enable(fits)
        return ctx

    def run(self, window=2, fits=FITS, never=False):
        key = (window, str(fits), never)
        if key not in self.cache:
            ctx = self.configured(window, fits, never=never)
            outs = ctx.batch_run(self.inputs, RATE, "ieee64")
            self.cache[key] = dict(outs=outs, tapfit=ctx.batch_tapfit() if fits and not never else None, report=ctx.batch_report(), kib=ctx.get_option("stat_batch_device_kib"))
            ctx.close()
        return self.cache[key]


@pytest.fixture(scope="module")
def job():
    return Job()


def test_batch_records_are_those_of_the_stand_alone_call_on_the_call_s_own_files(job, ctx1):
    run = job.run()
    rows = np.stack([o.view(np.float64) for o in run["outs"]])
    assert rows.shape == (NO + 1, BLOCKS * BLOCK) and np.isfinite(rows).all() and all(r.any() for r in rows[:NCH])
    assert run["tapfit"].shape == (BLOCKS, ref.list_doubles(FITS)) and run["tapfit"].any()
    same(run["tapfit"], ctx1.block_tapfit(rows, FITS, BLOCK), "batch against stand-alone")


def test_batch_records_are_the_same_bytes_however_the_job_is_cut(job):
    want = job.run(window=1)["tapfit"]
    same(job.run(window=2)["tapfit"], want, "window 2 against window 1")
    same(job.run(window=16)["tapfit"], want, "window 16 against window 1")
    for cuts in ((1, 2), (2, 1)):
        ctx = job.configured()
        parts = []
        for _ in ctx.batch_stream(job.inputs, RATE, "ieee64", lambda left: cuts[0] if left == BLOCKS else cuts[1]):
            parts.append(ctx.batch_tapfit())
        ctx.close()
        assert [p.shape[0] for p in parts] == list(cuts)
        same(np.concatenate(parts, axis=0), want, "slices of %d + %d" % cuts)


def test_checkpoint_resume_and_no_source_map_give_the_same_records(job):
    """the one file named three times instead of through a source map (a reader refuses the checkpoint calls), cut after the first block,
    resumed in a fresh context on which the fits are set again: the list is configuration, and the record is stateless"""
    want = job.run()["tapfit"]
    metas = [job.metas[0]] * NCH
    cut = lambda need: [job.file[2 * f:2 * (f + c)] for f, c in need]
    ctx = job.configured(source_map=False)
    assert ctx.batch_stream_open(metas, RATE, "ieee64") == BLOCKS * BLOCK
    ctx.batch_stream_step(1, cut(ctx.batch_stream_need(1)))
    head = ctx.batch_tapfit()
    blob = ctx.batch_stream_checkpoint()
    ctx.batch_stream_close()
    ctx.close()
    ctx = job.configured(source_map=False)
    assert ctx.batch_stream_resume(metas, RATE, "ieee64", blob) == BLOCK
    ctx.batch_stream_step(2, cut(ctx.batch_stream_need(2)))
    tail = ctx.batch_tapfit()
    ctx.batch_stream_close()
    ctx.close()
    same(np.concatenate([head, tail], axis=0), want, "checkpoint and resume, no source map")


def test_a_list_changes_no_output_byte_and_is_counted_and_off_is_never(job):
    on, never, off = job.run(window=2), job.run(window=2, never=True), job.run(window=2, fits=[])
    assert len(on["outs"]) == len(never["outs"]) == len(off["outs"]) == NO + 1
    for r in range(NO + 1):
        assert np.array_equal(on["outs"][r], never["outs"][r]) and np.array_equal(off["outs"][r], never["outs"][r]), r
    assert on["report"].tobytes() == never["report"].tobytes() == off["report"].tobytes()
    assert off["kib"] == never["kib"]
    # the table (9 ints per fit) and the room in each of the two download halves (16 + window x D doubles): the option counts whole KiB
    grown = 4 * 9 * len(FITS) + 2 * (16 + 2 * ref.list_doubles(FITS) * 8)
    assert grown // 1024 <= on["kib"] - never["kib"] <= -(-grown // 1024), (on["kib"], never["kib"], grown)
    ctx = job.configured()
    assert ctx.batch_tapfits() == len(FITS)
    ctx.batch_run(job.inputs, RATE, "ieee64")
    ctx.batch_tapfit_enable([])                                                  # off after having been on
    assert ctx.batch_tapfits() == 0
    outs = ctx.batch_run(job.inputs, RATE, "ieee64")
    with pytest.raises(job.pkg.GdgError, match="ran without them"):
        ctx.batch_tapfit()
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
    with pytest.raises(pkg.GdgError, match="no tap-fit records") as e:           # before any call
        ctx.batch_tapfit()
    assert e.value.code == pkg.GDG_ERR_INVALID
    for fits, what in (([(0, [1], 65)], "fit 0 has 65 taps per term"), ([(0, [1], 4), (0, [-1], 4)], "fit 1, term 0 names port -1"), ([(-2, [1], 4)], "fit 0 has the target port -2")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx.batch_tapfit_enable(fits)
        assert e.value.code == pkg.GDG_ERR_INVALID and ctx.batch_tapfits() == 0
    # a port at N + 3 + B: taken as configuration, refused and named when the job is described
    ctx.batch_tapfit_enable([(0, [1, NO + 1], 4)])
    with pytest.raises(pkg.GdgError, match="fit 0, term 1 names port %d" % (NO + 1)) as e:
        ctx.batch_run(job.inputs, RATE, "ieee64")
    assert e.value.code == pkg.GDG_ERR_INVALID
    ctx.batch_tapfit_enable([(NO + 1, [1], 4)])
    with pytest.raises(pkg.GdgError, match="fit 0 has the target port %d" % (NO + 1)):
        ctx.batch_stream_open(job.metas, RATE, "ieee64")
    with pytest.raises(pkg.GdgError, match="no tap-fit records"):
        ctx.batch_tapfit()
    # enabling while a streamed job is open: refused, and the list in force stays
    ctx.batch_tapfit_enable([(0, [1], 4)])
    ctx.batch_stream_open(job.metas, RATE, "ieee64")
    with pytest.raises(pkg.GdgError, match="a streamed batch run is open") as e:
        ctx.batch_tapfit_enable([(0, [2], 8)])
    assert e.value.code == pkg.GDG_ERR_INVALID and ctx.batch_tapfits() == 1
    ctx.batch_stream_close()
    ctx.close()
    # the shard calls, with fits on (and no blends, which they refuse first)
    ctx = job.configured(fits=[(0, [1], 4)])
    ctx.batch_set_blends([])
    for call, args in ((ctx.batch_run_shard, (job.inputs, RATE, "ieee64")), (ctx.batch_stream_open_shard, (job.metas, RATE, "ieee64"))):
        with pytest.raises(pkg.GdgError, match="1 tap fits are in force") as e:
            call(*args)
        assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    ctx.close()
