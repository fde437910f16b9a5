"""The Gram of a port list (include/gdg.h, GRAM) on the device.  The record kernel runs on the FP64 matrix instruction, so there is no
restatement of its sums in numpy (the four products of a step are fused).  What holds it instead: rows of small integers, whose every
partial sum is exact in any order -- the int64 Gram, bit for bit, for every tile shape and block length; random rows within L * 2^-52 *
sum |a b| of math.fsum; NaN sentinels around everything that may be addressed; the bits of an entry under everything the definition says
it does not depend on; and the batch form at 5 channels, 2 blends and 6 blocks: the same bytes whatever the window, the slicing, a
checkpoint and resume or a source map, and those of the stand-alone call on the call's own IEEE64 files."""
import math

import numpy as np
import pytest

from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
EPS = 2.0 ** -52
PS = [2, 16, 17, 64, 65, 130]                                                  # one tile; ragged tiles; three tile rows with off-diagonal tiles
CUTS = [(8192, 8192 + 5), (8191, 8191), (100, 250), (6, 15), (3, 7)]           # (block, samples): k tails that are no multiple of 4, odd lengths, a short last block


def tri(P):
    return np.tril_indices(P)


@pytest.fixture(scope="module")
def ctx1():
    ctx = package().Context(1, BLOCK)
    yield ctx
    ctx.close()


def listed(P, seed):
    """a list of P different rows out of P + 2, in no order: positions in the list are not row numbers"""
    return [int(p) for p in np.random.default_rng(seed).permutation(P + 2)[:P]]


def test_the_symbols_exist():
    pkg = package()
    for name in ("gdg_batch_gram_enable", "gdg_batch_gram_ports", "gdg_batch_gram", "gdg_block_gram_rows", "gdg_block_gram_rows_device", "gdg_blend_pick_from_gram"):
        assert getattr(pkg.lib(), name) is not None and name in pkg.ABI_SYMBOLS
    for name in ("batch_gram_enable", "batch_gram_ports", "batch_gram", "block_gram", "block_gram_device"):
        assert callable(getattr(pkg.Context, name))


# ---- 1. layout, exact -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PS)
def test_integer_rows_give_the_int64_gram_bit_for_bit(ctx1, P):
    """integers in [-8, 8]: a product is at most 64 and a sum of 8192 of them at most 2^19 -- every partial sum is an integer far below
    2^53, so any order, fused or not, is exact.  A wrong C/D row map, an exchange of row and column in an off-diagonal tile or a wrong
    packed index puts another integer there."""
    for block, samples in CUTS:
        rng = np.random.default_rng(1000 * P + block)
        xi = rng.integers(-8, 9, (P + 2, samples), dtype=np.int64)
        xi[:, 0] = np.arange(P + 2) % 17 - 8                                     # all rows different, in every first block
        xi[:, 1] = np.arange(P + 2) // 17
        ports = listed(P, P)
        got = ctx1.block_gram(xi.astype(np.float64), ports, block)
        blocks = -(-samples // block)
        assert got.shape == (blocks, P * (P + 1) // 2)
        for b in range(blocks):
            v = xi[ports, b * block:(b + 1) * block]
            want = (v @ v.T)[tri(P)].astype(np.float64)
            wrong = np.flatnonzero(got[b].view(np.uint64) != want.view(np.uint64))
            assert wrong.size == 0, "P %d, block %d of %d samples: %d of %d entries differ, the first at (i, j) = (%d, %d): %r, not %r" % (
                P, b, block, wrong.size, want.size, tri(P)[0][wrong[0]], tri(P)[1][wrong[0]], got[b][wrong[0]], want[wrong[0]])


def test_the_device_form_writes_the_records_and_nothing_behind_them(ctx1):
    P, block, samples = 65, 100, 250
    xi = np.random.default_rng(3).integers(-8, 9, (P, samples)).astype(np.float64)
    ports = list(range(P))
    want = ctx1.block_gram(xi, ports, block)
    d_rows, d_rec = ctx1.alloc(1, xi.size), ctx1.alloc(1, want.size + 1)
    d_rows.upload(xi.reshape(-1))
    d_rec.upload(np.full(want.size + 1, 7.0))
    ctx1.block_gram_device(d_rows.ptr, samples, P, samples, ports, d_rec.ptr, block)
    raw = d_rec.download().reshape(-1)
    d_rows.free()
    d_rec.free()
    assert raw[want.size] == 7.0, "the guard word behind the last record was written"
    assert raw[:want.size].tobytes() == want.tobytes()


# ---- 2. the error bound -----------------------------------------------------------------------------------------------------------------------
def random_rows(n_rows, samples, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.5, 1.5, (n_rows, samples))
    x[:, ::7] *= 1e-9
    return x


@pytest.mark.parametrize("P", PS)
def test_random_rows_lie_within_the_bound_of_fsum(ctx1, P):
    """every entry within L * 2^-52 * sum |a b| of math.fsum of the products, the bound tests/test_gpu_fit.py holds the fit's sums to: it
    holds for any order of L fused or unfused terms.  All entries where that is at most 2 million products, else the corners of every
    tile and 300 entries drawn once."""
    for block, samples in CUTS:
        x = random_rows(P + 2, samples, 77 * P + block)
        ports = listed(P, P + 1)
        got = ctx1.block_gram(x, ports, block)
        ii, jj = tri(P)
        if ii.size * samples > 2_000_000:
            pick = np.random.default_rng(P).choice(ii.size, 300, replace=False)
            edge = [e for e in range(ii.size) if ii[e] % 64 in (0, 63) and jj[e] % 64 in (0, 63)]
            pick = np.unique(np.concatenate([pick, edge, [ii.size - 1]])).astype(int)
        else:
            pick = np.arange(ii.size)
        for b in range(-(-samples // block)):
            v = x[ports, b * block:(b + 1) * block]
            L = v.shape[1]
            for e in pick:
                p = v[ii[e]] * v[jj[e]]
                exact, bound = math.fsum(p), L * EPS * math.fsum(np.abs(p))
                assert abs(got[b, e] - exact) <= bound, (P, block, b, int(ii[e]), int(jj[e]), got[b, e], exact, bound)


# ---- 3. padding -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,block,samples", [(17, 8192, 8192 + 5), (65, 100, 250), (130, 6, 15), (2, 3, 7)])
def test_nan_sentinels_around_the_addressed_range_change_nothing(ctx1, P, block, samples):
    """rows at an odd offset with a stride of samples + 3: NaN directly in front of the first row, between the rows, behind the last one,
    and a whole NaN row behind the last listed row -- one sample read outside [row, row + samples), or of a row that is not listed, and
    entries turn NaN"""
    x = random_rows(P, samples, 5 * P)
    ports = list(range(P))
    want = ctx1.block_gram(x, ports, block)
    assert np.isfinite(want).all()
    stride, off = samples + 3, 1
    padded = np.full(off + (P + 1) * stride + 2, np.nan)
    for r in range(P):
        padded[off + r * stride:off + r * stride + samples] = x[r]
    d_rows, d_rec = ctx1.alloc(1, padded.size), ctx1.alloc(1, want.size)
    d_rows.upload(padded)
    d_rec.upload(np.zeros(want.size))
    ctx1.block_gram_device(d_rows.ptr + 8 * off, stride, P + 1, samples, ports, d_rec.ptr, block)
    got = d_rec.download().reshape(want.shape)
    d_rows.free()
    d_rec.free()
    assert got.tobytes() == want.tobytes()


# ---- 4. the order, as defined -----------------------------------------------------------------------------------------------------------------
def test_an_entry_s_bits_do_not_depend_on_where_its_rows_stand(ctx1):
    """rows a and b of one set of random rows: the entries (a, b), (a, a) and (b, b) with the two rows alone, exchanged, inside a list of
    130 in one diagonal tile, in an off-diagonal tile, across a tile border, and with the pair exchanged there"""
    samples = BLOCK + 5
    x = random_rows(130, samples, 404)
    a, b = 5, 77
    others = [r for r in range(130) if r not in (a, b)]

    def at(pos_a, pos_b, P):
        ports = others[:P - 2]
        for pos, row in sorted([(pos_a, a), (pos_b, b)]):
            ports.insert(pos, row)
        rec = ctx1.block_gram(x, ports, BLOCK)
        pkg = package()
        return np.stack([rec[:, pkg.gram_index(pos_a, pos_b)], rec[:, pkg.gram_index(pos_a, pos_a)], rec[:, pkg.gram_index(pos_b, pos_b)]])

    want = at(0, 1, 2)
    assert want.shape == (3, 2) and np.isfinite(want).all()
    for pos_a, pos_b, P in ((1, 0, 2), (3, 40, 130), (40, 3, 130), (3, 100, 130), (100, 3, 130), (63, 64, 65), (64, 63, 65), (129, 0, 130), (16, 15, 17)):
        got = at(pos_a, pos_b, P)
        assert got.tobytes() == want.tobytes(), (pos_a, pos_b, P, got, want)


def test_a_list_is_checked_before_anything_is_launched(ctx1):
    pkg = package()
    x = random_rows(3, 64, 1)
    for ports, what in (([0, 3], "list entry 1 names row 3 of 3"), ([0, -1], "list entry 1 names row -1 of 3"), ([1, 2, 1], "list entry 2 names port 1, which entry 0 names already"),
                        ([], "a list of 0 ports; 1 to 512")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx1.block_gram(x, ports)
        assert e.value.code == pkg.GDG_ERR_INVALID
    with pytest.raises(pkg.GdgError, match="blocks of 0 samples"):
        ctx1.block_gram(x, [0, 1], 0)


# ---- 5. the batch form ------------------------------------------------------------------------------------------------------------------------
RATE, NCH, BLOCKS = 48000, 5, 6
SAMPLES = 5 * BLOCK + 1000
NO = NCH + 3
BLENDS = [[(0, 0.6), (1, -0.3)], [(2, 1.0), (4, 0.5)]]                          # ports NO and NO + 1
LIST = [NO + 1, 0, 3, NO, NCH, 1, NCH + 1, 4]                                   # both blends, four chain outputs, master left and right


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    """5 channels on one source with power amps of different random taps"""

    def __init__(self):
        self.pkg = package()
        self.file = lpcm16_file(0.1 * synth_signal(0, SAMPLES, RATE) + 0.2 * np.random.default_rng(11).uniform(-1.0, 1.0, SAMPLES))
        self.inputs = [(self.file, "lpcm16", RATE)] + [None] * (NCH - 1)
        self.metas = [(SAMPLES, "lpcm16", RATE)] + [None] * (NCH - 1)
        self.irs = [synth_ir(n, seed=530 + c) for c, n in enumerate((300, 64, 128, 200, 96))]
        self.cache = {}

    def configured(self, window=2, gram=LIST, source_map=True):
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
        if gram is not None:
            ctx.batch_gram_enable(gram)
        return ctx

    def run(self, window=2, gram=LIST):
        key = (window, str(gram))
        if key not in self.cache:
            ctx = self.configured(window, gram)
            outs = ctx.batch_run(self.inputs, RATE, "ieee64")
            self.cache[key] = dict(outs=outs, gram=ctx.batch_gram() if gram else None, report=ctx.batch_report(), kib=ctx.get_option("stat_batch_device_kib"))
            ctx.close()
        return self.cache[key]


@pytest.fixture(scope="module")
def job():
    return Job()


def same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), "%s: %d of %d entries differ" % (what, np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)), got.size)


def test_batch_records_are_those_of_the_stand_alone_call_on_the_call_s_own_files(job, ctx1):
    run = job.run()
    rows = np.stack([o.view(np.float64) for o in run["outs"]])
    assert rows.shape == (NO + 2, BLOCKS * BLOCK) and np.isfinite(rows).all() and all(r.any() for r in rows[:NCH])
    P = len(LIST)
    assert run["gram"].shape == (BLOCKS, P * (P + 1) // 2)
    same(run["gram"], ctx1.block_gram(rows, LIST, BLOCK), "batch against stand-alone")
    ii, jj = tri(P)
    for b in (0, BLOCKS - 1):                                                    # ... and the fsum bound once more, on rendered audio
        v = rows[LIST, b * BLOCK:(b + 1) * BLOCK]
        for e in range(ii.size):
            p = v[ii[e]] * v[jj[e]]
            assert abs(run["gram"][b, e] - math.fsum(p)) <= BLOCK * EPS * math.fsum(np.abs(p)), (b, e)


def test_batch_records_are_the_same_bytes_however_the_job_is_cut(job):
    want = job.run(window=1)["gram"]
    same(job.run(window=4)["gram"], want, "window 4 against window 1")
    same(job.run(window=2)["gram"], want, "window 2 against window 1")
    ctx = job.configured()
    parts = []
    for _ in ctx.batch_stream(job.inputs, RATE, "ieee64", lambda left: {BLOCKS: 1, BLOCKS - 1: 2}.get(left, 3)):
        parts.append(ctx.batch_gram())
    ctx.close()
    assert [p.shape[0] for p in parts] == [1, 2, 3]
    same(np.concatenate(parts, axis=0), want, "slices of 1 + 2 + 3")


def test_checkpoint_resume_and_no_source_map_give_the_same_records(job):
    """the one file named five times instead of through a source map (a reader refuses the checkpoint calls), cut in the middle, resumed
    in a fresh context on which the list is set again: a list is configuration, and a Gram is stateless"""
    want = job.run()["gram"]
    metas = [job.metas[0]] * NCH
    cut = lambda need: [job.file[2 * f:2 * (f + c)] for f, c in need]
    ctx = job.configured(source_map=False)
    assert ctx.batch_stream_open(metas, RATE, "ieee64") == BLOCKS * BLOCK
    ctx.batch_stream_step(3, cut(ctx.batch_stream_need(3)))
    head = ctx.batch_gram()
    blob = ctx.batch_stream_checkpoint()
    ctx.batch_stream_close()
    ctx.close()
    ctx = job.configured(source_map=False)
    assert ctx.batch_stream_resume(metas, RATE, "ieee64", blob) == 3 * BLOCK
    ctx.batch_stream_step(3, cut(ctx.batch_stream_need(3)))
    tail = ctx.batch_gram()
    ctx.batch_stream_close()
    ctx.close()
    same(np.concatenate([head, tail], axis=0), want, "checkpoint and resume, no source map")


def test_a_list_changes_no_output_byte_and_is_counted(job):
    on, never = job.run(window=2), job.run(window=2, gram=None)
    assert len(on["outs"]) == len(never["outs"]) == NO + 2
    for r in range(NO + 2):
        assert np.array_equal(on["outs"][r], never["outs"][r]), r
    assert on["report"].tobytes() == never["report"].tobytes()
    # the list (P ints) and the room in each of the two download halves (16 + window x P (P + 1) / 2 doubles): the option counts whole KiB
    P = len(LIST)
    grown = 4 * P + 2 * (16 + 2 * (P * (P + 1) // 2) * 8)
    assert grown // 1024 <= on["kib"] - never["kib"] <= -(-grown // 1024), (on["kib"], never["kib"], grown)
    ctx = job.configured()
    assert ctx.batch_gram_ports() == LIST
    ctx.batch_run(job.inputs, RATE, "ieee64")
    ctx.batch_gram_enable([])                                                    # off after having been on
    assert ctx.batch_gram_ports() == []
    outs = ctx.batch_run(job.inputs, RATE, "ieee64")
    with pytest.raises(job.pkg.GdgError, match="ran without them"):
        ctx.batch_gram()
    kib = ctx.get_option("stat_batch_device_kib")
    ctx.close()
    fresh = job.configured(gram=None)
    fresh.batch_run(job.inputs, RATE, "ieee64")
    want_outs = fresh.batch_run(job.inputs, RATE, "ieee64")                      # the second job of a context, as above
    assert kib == fresh.get_option("stat_batch_device_kib")
    fresh.close()
    for r in range(NO + 2):
        assert np.array_equal(outs[r], want_outs[r]), r


def test_refusals(job):
    pkg = job.pkg
    ctx = job.configured(gram=None)
    with pytest.raises(pkg.GdgError, match="no Gram records") as e:              # before any call
        ctx.batch_gram()
    assert e.value.code == pkg.GDG_ERR_INVALID
    for ports, what in (([3], "a list of 1 ports; 2 to 512"), (list(range(513)), "a list of 513 ports"), ([0, -1], "list entry 1 names port -1"),
                        ([0, 4, 0], "list entry 2 names port 0, which entry 0 names already")):
        with pytest.raises(pkg.GdgError, match=what) as e:
            ctx.batch_gram_enable(ports)
        assert e.value.code == pkg.GDG_ERR_INVALID and ctx.batch_gram_ports() == []
    # a port at N + 3 + B: taken as configuration, refused and named when the job is described
    ctx.batch_gram_enable([0, NO + 2])
    with pytest.raises(pkg.GdgError, match="list entry 1 names port %d" % (NO + 2)) as e:
        ctx.batch_run(job.inputs, RATE, "ieee64")
    assert e.value.code == pkg.GDG_ERR_INVALID
    with pytest.raises(pkg.GdgError, match="list entry 1 names port %d" % (NO + 2)):
        ctx.batch_stream_open(job.metas, RATE, "ieee64")
    with pytest.raises(pkg.GdgError, match="no Gram records"):
        ctx.batch_gram()
    ctx.close()
    # the shard calls, with a list on (and no blends, which they refuse first)
    ctx = job.configured(gram=[0, 1])
    ctx.batch_set_blends([])
    with pytest.raises(pkg.GdgError, match="a Gram list of 2 ports is in force") as e:
        ctx.batch_run_shard(job.inputs, RATE, "ieee64")
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    with pytest.raises(pkg.GdgError, match="a Gram list of 2 ports is in force") as e:
        ctx.batch_stream_open_shard(job.metas, RATE, "ieee64")
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    ctx.close()
