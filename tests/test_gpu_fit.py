"""The blend fit (include/gdg.h, FIT) on the device.  The record kernel bit for bit against a numpy restatement of the order of its sums --
the per-thread walk over sample pairs, the lane tree, the four waves in order; numpy's float64 products and adds are the rounded ones, so
the restatement is exact -- and, independently, every sum within n * 2^-52 * sum|a_i b_i| of math.fsum of the rounded products.  The
stand-alone form at every block length at which a path changes (1, 63, 64, 65, 1000, 8192, each with a short last block) for 1, 2 and 8
terms; the batch form at 3 channels on one source and 5 blocks: the records against the call's own IEEE64 files and its block statistics,
the planner's known answer, and the same bytes whatever the window, the slicing or a checkpoint and resume."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
T = 256                                                                         # threads of a workgroup
EPS = 2.0 ** -52


# ---- the order of the sums, restated (exact: numpy multiplies and adds float64 with one rounding each) --------------------------------------
def ordered_sum(p):
    """products p of one block, +0.0 where a sample is skipped (a running sum is never -0.0, so adding +0.0 is adding nothing) -> the
    kernel's sum: thread t adds the samples 2 q and 2 q + 1 of the pairs q = t, t + 256 ..; lane i <- lane i + 32, 16 .. 1; waves 0, 1, 2, 3"""
    n = -(-p.size // (2 * T)) * 2 * T
    q = np.zeros(n)
    q[:p.size] = p
    q = q.reshape(-1, T, 2)
    acc = np.zeros(T)
    for r in range(q.shape[0]):
        acc = acc + q[r, :, 0]
        acc = acc + q[r, :, 1]
    waves = acc.reshape(4, 64).copy()
    o = 32
    while o:
        waves[:, :o] = waves[:, :o] + waves[:, o:2 * o]
        o >>= 1
    return ((waves[0, 0] + waves[1, 0]) + waves[2, 0]) + waves[3, 0]


def entries(K):
    """(field, index, row a, row b) of a fit's live sums, rows numbered 0 = target, 1 + k = term k"""
    out = [("tt", None, 0, 0)] + [("tx", k, 0, 1 + k) for k in range(K)]
    return out + [("xx", j * (j + 1) // 2 + k, 1 + j, 1 + k) for j in range(K) for k in range(j + 1)]


def restated(rows, fits, block, pkg):
    """the records of `fits` over `rows` as the kernel's order gives them, and per sum the fsum of the products and its bound"""
    samples = rows.shape[1]
    blocks = -(-samples // block)
    rec = np.zeros((len(fits), blocks), dtype=pkg.FIT_DTYPE)
    exact, bound = {}, {}
    with np.errstate(invalid="ignore", over="ignore"):
        for f, (target, ports) in enumerate(fits):
            K = len(ports)
            for b in range(blocks):
                v = rows[[target] + list(ports), b * block:(b + 1) * block]
                ok = np.isfinite(v).all(axis=0)
                rec[f, b]["skipped"], rec[f, b]["terms"] = np.count_nonzero(~ok), K
                for field, idx, ra, rb in entries(K):
                    p = np.where(ok, v[ra] * v[rb], 0.0)
                    s = ordered_sum(p)
                    if idx is None:
                        rec[f, b][field] = s
                    else:
                        rec[f, b][field][idx] = s
                    exact[(f, b, field, idx)] = math.fsum(p)
                    bound[(f, b, field, idx)] = int(ok.sum()) * EPS * math.fsum(np.abs(p))
    return rec, exact, bound


def same_records(got, want, what):
    assert got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), "%s: %d of %d records differ" % (what, np.count_nonzero(got != want), got.size)


def within_fsum(got, fits, exact, bound, what):
    for f, (_, ports) in enumerate(fits):
        for b in range(got.shape[1]):
            for field, idx, _, _ in entries(len(ports)):
                v = got[f, b][field] if idx is None else got[f, b][field][idx]
                key = (f, b, field, idx)
                assert abs(v - exact[key]) <= bound[key], (what, key, v, exact[key], bound[key])


def tail_is_zero(got, fits):
    for f, (_, ports) in enumerate(fits):
        K = len(ports)
        assert (got[f]["terms"] == K).all()
        for name, live in (("tx", K), ("xx", K * (K + 1) // 2)):
            tail = got[f][name][:, live:]
            assert not tail.any() and not np.signbit(tail).any(), (f, name)         # +0.0, not -0.0


# ---- the symbols ----------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_exist():
    pkg = package()
    for name in ("gdg_batch_fit_enable", "gdg_batch_fits", "gdg_batch_fit", "gdg_block_fit_rows", "gdg_block_fit_rows_device", "gdg_blend_weights_from_fit"):
        assert getattr(pkg.lib(), name) is not None and name in pkg.ABI_SYMBOLS
    assert pkg.FIT_DTYPE.itemsize == 368 and pkg.FIT_MAX_TERMS == 8
    for name in ("batch_fit_enable", "batch_fits", "batch_fit", "block_fit", "block_fit_device"):
        assert callable(getattr(pkg.Context, name))
    assert callable(pkg.blend_weights_from_fit)


# ---- the stand-alone form -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


def random_rows(n_rows, samples, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, (n_rows, samples))
    x[:, ::7] *= 1e-9
    return x


# nine rows; fits of 1, 2 and 8 terms: a target that is a term, a port twice, every row used
FITS = [(8, [3]), (0, [0, 5]), (4, [0, 1, 2, 3, 5, 6, 7, 1])]


@pytest.mark.parametrize("block,samples", [(1, 3), (63, 2 * 63 + 5), (64, 2 * 64 + 1), (65, 2 * 65 + 7), (1000, 2300), (8192, 8192 + 777)])
def test_standalone_records_are_the_restatement_bit_for_bit(ctx1, block, samples):
    pkg = package()
    x = random_rows(9, samples, 40 + block)
    want, exact, bound = restated(x, FITS, block, pkg)
    got = ctx1.block_fit(x, FITS, block)
    same_records(got, want, "block %d" % block)
    within_fsum(got, FITS, exact, bound, "block %d" % block)
    tail_is_zero(got, FITS)
    assert not got["skipped"].any()
    # the device form, with a guard word behind the last record
    n_rec = got.size * 46
    d_rows, d_rec = ctx1.alloc(1, x.size), ctx1.alloc(1, n_rec + 1)
    d_rows.upload(x.reshape(-1))
    d_rec.upload(np.full(n_rec + 1, 7.0))
    ctx1.block_fit_device(d_rows.ptr, samples, 9, samples, FITS, d_rec.ptr, block)
    raw = d_rec.download().reshape(-1)
    assert raw[n_rec] == 7.0, "the guard word behind the last record was written"
    assert raw[:n_rec].tobytes() == want.tobytes()
    d_rows.free()
    d_rec.free()


def test_alignment_and_stride_do_not_change_a_bit(ctx1):
    """8192 samples at a 16-byte-aligned base with an even stride (16-byte loads) and at an odd offset with an odd stride (8-byte loads)"""
    pkg = package()
    samples = BLOCK
    x = random_rows(3, samples, 7)
    fits = [(2, [0, 1])]
    want, _, _ = restated(x, fits, BLOCK, pkg)
    raws = []
    for off, stride in ((0, samples), (1, samples + 1)):
        d_rows, d_rec = ctx1.alloc(1, 3 * stride + 2), ctx1.alloc(1, 46)
        padded = np.full(3 * stride + 2, np.nan)                                # a sample outside a row that was read would be skipped, and counted
        for r in range(3):
            padded[off + r * stride:off + r * stride + samples] = x[r]
        d_rows.upload(padded)
        d_rec.upload(np.zeros(46))
        ctx1.block_fit_device(d_rows.ptr + 8 * off, stride, 3, samples, fits, d_rec.ptr, BLOCK)
        raws.append(d_rec.download().reshape(-1).tobytes())
        d_rows.free()
        d_rec.free()
    assert raws[0] == raws[1] == want.tobytes()


def test_symmetry_under_exchange_and_a_repeated_term(ctx1):
    x = random_rows(4, 2 * BLOCK + 11, 21)
    a, b = ctx1.block_fit(x, [(3, [0, 1, 2]), (3, [1, 0, 2])])
    at = lambda j, k: (j * (j + 1) // 2 + k) if k <= j else (k * (k + 1) // 2 + j)
    swap = [1, 0, 2]
    for j in range(3):
        assert a["tx"][:, j].tobytes() == b["tx"][:, swap[j]].tobytes()
        for k in range(3):
            assert a["xx"][:, at(j, k)].tobytes() == b["xx"][:, at(swap[j], swap[k])].tobytes(), (j, k)
    assert a["tt"].tobytes() == b["tt"].tobytes()
    # a term twice: equal rows and columns
    r, = ctx1.block_fit(x, [(3, [0, 1, 0])])
    assert r["tx"][:, 0].tobytes() == r["tx"][:, 2].tobytes()
    assert r["xx"][:, at(0, 0)].tobytes() == r["xx"][:, at(2, 2)].tobytes() == r["xx"][:, at(2, 0)].tobytes()
    assert r["xx"][:, at(1, 0)].tobytes() == r["xx"][:, at(2, 1)].tobytes()


def test_nonfinite_samples_are_skipped_in_every_sum(ctx1):
    pkg = package()
    samples = BLOCK + 300
    x = random_rows(4, samples, 33)
    fits = [(3, [0, 1, 2]), (0, [1])]
    x[1, 100] = np.nan                                                          # a term's row
    x[3, 5000] = np.inf                                                         # the target's row
    x[1, BLOCK + 7] = -np.inf                                                   # the second block
    got = ctx1.block_fit(x, fits)
    want, _, _ = restated(x, fits, BLOCK, pkg)
    same_records(got, want, "with NaN and inf")
    assert got["skipped"].tolist() == [[2, 1], [1, 1]]                          # fit 1 reads rows 0 and 1 alone
    # ... and equal the sums of the rows with those indices deleted: another walk over the samples, so within the fsum bound of both
    keep = np.ones(samples, dtype=bool)
    keep[[100, 5000]] = False
    first = x[:, :BLOCK][:, keep[:BLOCK]]
    for field, idx, ra, rb in entries(3):
        rows = [3, 0, 1, 2]
        p = first[rows[ra]] * first[rows[rb]]
        v = got[0, 0][field] if idx is None else got[0, 0][field][idx]
        assert np.isfinite(v) and abs(v - math.fsum(p)) <= p.size * EPS * math.fsum(np.abs(p)), (field, idx)


def test_standalone_refusals_name_the_fit(ctx1):
    pkg = package()
    x = np.ones((2, 8))
    for fits, what in (([(0, [0]), (1, [0, 2])], "fit 1, term 1 names row 2"), ([(2, [0])], "fit 0 has the target row 2"), ([(0, [])], "fit 0 has 0 terms"),
                       ([(0, [0] * 9)], "fit 0 has 9 terms")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx1.block_fit(x, fits)
        assert e.value.code == pkg.GDG_ERR_INVALID
    with pytest.raises(pkg.GdgError, match="blocks of 0 samples"):
        ctx1.block_fit(x, [(0, [1])], 0)


# ---- the batch form -------------------------------------------------------------------------------------------------------------------------
RATE, NCH, BLOCKS = 48000, 3, 5
SAMPLES = 4 * BLOCK + 1000
NO = NCH + 3
A = [(0, 0.6), (1, -0.3)]                                                       # port NO: the known answer's target
DELAYED = [A, [(2, 1.0, 5)]]                                                    # port NO + 1: channel 2, five samples late
PLAIN = [A, [(2, 1.0)]]
FITS_B = [(NO, [0, 1]), (0, [0, 1, NO + 1])]


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """3 channels on one source with power amps of 300, 64 and 128 random taps: three renders of one take that differ enough"""

    def __init__(self):
        self.pkg = package()
        # a take with a broad spectrum: two sines alone would leave every render in one four-dimensional space, and the fits ill-posed
        self.file = lpcm16_file(0.1 * synth_signal(0, SAMPLES, RATE) + 0.2 * np.random.default_rng(11).uniform(-1.0, 1.0, SAMPLES))
        self.inputs = [(self.file, "lpcm16", RATE), None, None]
        self.metas = [(SAMPLES, "lpcm16", RATE), None, None]
        self.irs = [synth_ir(n, seed=230 + c) for c, n in enumerate((300, 64, 128))]
        self.cache = {}

    def configured(self, window=2, blends=DELAYED, fits=FITS_B, report=True, source_map=True):
        ctx = self.pkg.Context(NCH, BLOCK)
        for c in range(NCH):
            ctx.append_unit(c, "power_amp", fir=self.irs[c])
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(NCH):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * c, 1.0 + 0.5 * c, 0.8)
        ctx.set_window(window)
        if source_map:
            ctx.batch_set_sources([0, 0, 0])
        if blends is not None:
            ctx.batch_set_blends(blends)
        if report:
            ctx.batch_report_enable(True)
        if fits is not None:
            ctx.batch_fit_enable(fits)
        return ctx

    def run(self, window=2, blends=DELAYED, fits=FITS_B):
        key = (window, str(blends), str(fits))
        if key not in self.cache:
            ctx = self.configured(window, blends, fits)
            outs = ctx.batch_run(self.inputs, RATE, "ieee64")
            self.cache[key] = dict(outs=outs, fit=ctx.batch_fit() if fits else None, report=ctx.batch_report(), kib=ctx.get_option("stat_batch_device_kib"))
            ctx.close()
        return self.cache[key]

    def cut(self, need):
        return [None if d is None else self.file[2 * f:2 * (f + c)] for d, (f, c) in zip(self.inputs, need)]


@pytest.fixture(scope="module")
def job():
    return Job()


def test_known_answer_fit_in_a_batch_run(job):
    pkg = job.pkg
    run = job.run()
    rows = np.stack([o.view(np.float64) for o in run["outs"]])
    assert rows.shape == (NO + 2, BLOCKS * BLOCK) and np.isfinite(rows).all() and all(r.any() for r in rows[:NCH])
    fit, report = run["fit"], run["report"]
    assert fit.shape == (2, BLOCKS) and report.shape == (NO + 2, BLOCKS) and not fit["skipped"].any()
    tail_is_zero(fit, FITS_B)
    # the diagonal and tt: the block statistics' sum_sq of that port, bit for bit
    for f, (target, ports) in enumerate(FITS_B):
        assert fit[f]["tt"].tobytes() == report[target]["sum_sq"].tobytes(), f
        for k, p in enumerate(ports):
            assert fit[f]["xx"][:, k * (k + 1) // 2 + k].tobytes() == report[p]["sum_sq"].tobytes(), (f, k)
    # every entry: the restatement over the decoded files (the blend ports' own files), and the fsum bound
    want, exact, bound = restated(rows, FITS_B, BLOCK, pkg)
    same_records(fit, want, "batch")
    within_fsum(fit, FITS_B, exact, bound, "batch")
    # the two chain outputs differ enough for the known answer to be well posed
    G = np.array([[math.fsum(rows[j] * rows[k]) for k in range(2)] for j in range(2)])
    assert np.linalg.cond(G) <= 1e3, np.linalg.cond(G)
    G3 = np.array([[math.fsum(rows[j] * rows[k]) for k in (0, 1, NO + 1)] for j in (0, 1, NO + 1)])
    assert np.linalg.cond(G3) <= 1e3, np.linalg.cond(G3)
    w, res = pkg.blend_weights_from_fit(fit)
    assert abs(w[0, 0] - 0.6) <= 1e-9 and abs(w[0, 1] + 0.3) <= 1e-9 and not w[0, 2:].any() and res[0] <= 1e-12, (w[0], res[0])
    # fit 2: port 0 is its own first term
    assert abs(w[1, 0] - 1.0) <= 1e-9 and abs(w[1, 1]) <= 1e-9 and abs(w[1, 2]) <= 1e-9 and res[1] <= 1e-12, (w[1], res[1])


def test_records_are_the_same_bytes_however_the_job_is_cut(job):
    want = job.run()["fit"]
    for window in (1, 4):
        same_records(job.run(window=window)["fit"], want, "window %d" % window)
    ctx = job.configured()
    parts = []
    for _ in ctx.batch_stream(job.inputs, RATE, "ieee64", lambda left: 2 if left == BLOCKS else 3):
        parts.append(ctx.batch_fit())
    ctx.close()
    assert [p.shape for p in parts] == [(2, 2), (2, 3)]
    same_records(np.concatenate(parts, axis=1), want, "slices of 2 + 3")


def test_checkpoint_and_resume_with_fits_on(job):
    """the checkpointed job carries undelayed blends only and names the one file three times instead of through a source map (a delay and a
    reader refuse the checkpoint calls, as ever); fits are configuration: set again on the target.  The records are those of the job with
    the source map, run in one call."""
    want = job.run(blends=PLAIN)["fit"]
    inputs, metas = [job.inputs[0]] * NCH, [job.metas[0]] * NCH
    cut = lambda need: [job.file[2 * f:2 * (f + c)] for f, c in need]
    ctx = job.configured(blends=PLAIN, source_map=False)
    assert ctx.batch_stream_open(metas, RATE, "ieee64") == BLOCKS * BLOCK
    ctx.batch_stream_step(2, cut(ctx.batch_stream_need(2)))
    head = ctx.batch_fit()
    blob = ctx.batch_stream_checkpoint()
    ctx.batch_stream_close()
    ctx.close()
    ctx = job.configured(blends=PLAIN, source_map=False)
    assert ctx.batch_stream_resume(metas, RATE, "ieee64", blob) == 2 * BLOCK
    ctx.batch_stream_step(3, cut(ctx.batch_stream_need(3)))
    tail = ctx.batch_fit()
    ctx.batch_stream_close()
    ctx.close()
    same_records(np.concatenate([head, tail], axis=1), want, "checkpoint and resume")


def test_refusals(job):
    pkg = job.pkg
    ctx = job.configured(fits=None)
    with pytest.raises(pkg.GdgError, match="no fit records") as e:               # before any call
        ctx.batch_fit()
    assert e.value.code == pkg.GDG_ERR_INVALID
    for fits, what in (([(0, [])], "fit 0 has 0 terms"), ([(0, [0]), (1, [0] * 9)], "fit 1 has 9 terms"), ([(0, [0, -1])], "fit 0, term 1 names port -1")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx.batch_fit_enable(fits)
        assert e.value.code == pkg.GDG_ERR_INVALID and ctx.batch_fits() == 0
    # a port at N + 3 + B: taken as configuration, refused and named when the job is described
    ctx.batch_fit_enable([(0, [1]), (1, [0, NO + 2])])
    assert ctx.batch_fits() == 2
    with pytest.raises(pkg.GdgError, match="fit 1, term 1 names port %d" % (NO + 2)) as e:
        ctx.batch_run(job.inputs, RATE, "ieee64")
    assert e.value.code == pkg.GDG_ERR_INVALID
    ctx.batch_fit_enable([(NO + 2, [0])])
    with pytest.raises(pkg.GdgError, match="fit 0 has the target port %d" % (NO + 2)):
        ctx.batch_stream_open(job.metas, RATE, "ieee64")
    with pytest.raises(pkg.GdgError, match="no fit records"):
        ctx.batch_fit()
    ctx.close()
    # the shard calls, with fits on (and no blends, which they refuse first)
    ctx = job.configured(blends=None, fits=[(0, [1])])
    with pytest.raises(pkg.GdgError, match="fits are in force") as e:
        ctx.batch_run_shard(job.inputs, RATE, "ieee64")
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    with pytest.raises(pkg.GdgError, match="fits are in force") as e:
        ctx.batch_stream_open_shard(job.metas, RATE, "ieee64")
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    ctx.close()


def test_off_is_a_context_that_never_heard_of_it(job):
    never = job.run(fits=None)
    assert job.run()["kib"] > never["kib"]                                       # on: the table and the records' room are counted
    ctx = job.configured()
    ctx.batch_true_peak_enable(True)
    ctx.batch_run(job.inputs, RATE, "ieee64")
    ctx.batch_fit_enable([])                                                     # off after having been on
    assert ctx.batch_fits() == 0
    outs = ctx.batch_run(job.inputs, RATE, "ieee64")
    got = dict(report=ctx.batch_report(), tp=ctx.batch_true_peak(), kib=ctx.get_option("stat_batch_device_kib"))
    with pytest.raises(job.pkg.GdgError, match="ran without them"):
        ctx.batch_fit()
    ctx.close()
    fresh = job.configured(fits=None)
    fresh.batch_true_peak_enable(True)
    fresh.batch_run(job.inputs, RATE, "ieee64")
    want_outs = fresh.batch_run(job.inputs, RATE, "ieee64")                      # the second job of a context, as above
    want = dict(report=fresh.batch_report(), tp=fresh.batch_true_peak(), kib=fresh.get_option("stat_batch_device_kib"))
    fresh.close()
    assert got["kib"] == want["kib"]
    assert got["report"].tobytes() == want["report"].tobytes() and got["tp"].tobytes() == want["tp"].tobytes()
    for r in range(len(want_outs)):
        assert np.array_equal(outs[r], want_outs[r]), r
    # ... and the files of the job with fits on are those of the job without
    for r in range(len(never["outs"])):
        assert np.array_equal(job.run()["outs"][r], never["outs"][r]), r
