"""The streamed form of a SHARD (gdg_batch_stream_open_shard / gdg_batch_stream_step_shard) and the per-slice finish of the master
(gdg_batch_finish_master_slice).  The yardstick is the one-call form on fresh, identically configured contexts -- gdg_batch_run_shard
per shard, then gdg_batch_finish_master -- byte for byte: the same kernels in the same order (the finish: the same adds in the same
order, then the same encoder), so no tolerance anywhere; beside it the oracle pipeline under the one-call sharded test's own rules.
The finish alone: both entry points run one engine, so each is held against numpy's float64 sums in the documented order, the oracle's
encoder, a third context's meters and block_stats of the sums -- exact equality as well."""
import numpy as np
import pytest

from helpers import TOL_RMS, package, rms
from test_gpu_batch_stream import BLOCK, FORMATS, _long_job, _plain_job, after_job, batch_case, pkg_width, random_slicing, same_tuners

pytestmark = pytest.mark.gpu

SPLIT = [(0, 2), (2, 2), (4, 1)]                 # batch_case's five channels over three contexts; the last one's file is two blocks long
KW = dict(run_meters=True, tuner_enqueue=True)


def one_call_sharded(ctxs, split, inputs, rate, out_fmt, job, finish_on=0):
    """gdg_batch_run_shard per context, then gdg_batch_finish_master: (outs + [left, right, metronome], per-shard results)"""
    shards = [ctx.batch_run_shard(inputs[f:f + n], rate, out_fmt, job_samples=job, metronome=(g == 0), **KW) for g, (ctx, (f, n)) in enumerate(zip(ctxs, split))]
    ml, mr = ctxs[finish_on].batch_finish_master(out_fmt, [s[1] for s in shards], [s[2] for s in shards], aux=shards[0][4], sample_rate=rate, run_meters=True)
    return sum((s[0] for s in shards), []) + [ml, mr, shards[0][3]], shards


def streamed_sharded(ctxs, split, inputs, rate, out_fmt, job, slicing, finish_on=0):
    """every shard sliced alike, each slice's master finished with gdg_batch_finish_master_slice; the same shapes as one_call_sharded"""
    wo = pkg_width(out_fmt)
    gens = []
    for g, (ctx, (f, n)) in enumerate(zip(ctxs, split)):
        it = iter(slicing)
        gens.append(ctx.batch_stream_shard(inputs[f:f + n], rate, out_fmt, lambda left, it=it: next(it), job_samples=job, metronome=(g == 0), **KW))
    slices, masters = [], []
    for k in slicing:
        parts = [next(gen) for gen in gens]
        for g, p in enumerate(parts):
            assert [o.size for o in p[0]] == [k * BLOCK * wo] * split[g][1] and p[1].size == p[2].size == k * BLOCK
            assert (p[3] is None) == (g != 0) and (p[4] is None) == (g != 0)
        masters.append(ctxs[finish_on].batch_finish_master_slice(out_fmt, [p[1] for p in parts], [p[2] for p in parts], aux=parts[0][4], sample_rate=rate, run_meters=True))
        slices.append(parts)
    for gen in gens:
        with pytest.raises(StopIteration):
            next(gen)                                               # the job is done: the generator closes it
    shards = []
    for g in range(len(ctxs)):
        outs = [np.concatenate([s[g][0][c] for s in slices]) for c in range(split[g][1])]
        row = lambda r: None if slices[0][g][r] is None else np.concatenate([s[g][r] for s in slices])
        shards.append((outs, row(1), row(2), row(3), row(4)))
    ml, mr = np.concatenate([m[0] for m in masters]), np.concatenate([m[1] for m in masters])
    return sum((s[0] for s in shards), []) + [ml, mr, shards[0][3]], shards


def same_shards(got, want, what):
    for g, (a, b) in enumerate(zip(got, want)):
        for c, (x, y) in enumerate(zip(a[0], b[0])):
            assert np.array_equal(x, y), "%s: shard %d, chain output %d" % (what, g, c)
        for r, name in ((1, "left partial"), (2, "right partial"), (3, "metronome file"), (4, "float64 metronome")):
            assert (a[r] is None) == (b[r] is None), (what, g, name)
            if a[r] is not None:
                assert a[r].dtype == b[r].dtype and np.array_equal(a[r].view(np.uint8), b[r].view(np.uint8)), "%s: shard %d, %s" % (what, g, name)


@pytest.mark.parametrize("W", [1, 2, 8])
@pytest.mark.parametrize("out_fmt", ["lpcm24", "ieee64"])
def test_sliced_shards_have_the_bytes_of_the_one_call_shards(oracle, out_fmt, W):
    case = batch_case(oracle)
    rate, nch, inputs, job = case.rate, case.nch, case.inputs, case.length
    assert job == 9 * BLOCK

    def contexts():
        ctxs = [case.configured(f, n) for f, n in SPLIT]
        for ctx in ctxs:
            ctx.set_window(W)
        return ctxs

    ctxs = contexts()
    assert ctxs[2].batch_length(inputs[4:5], rate) == 2 * BLOCK                  # shard 2 pads beyond its own length
    want, want_shards = one_call_sharded(ctxs, SPLIT, inputs, rate, out_fmt, job)
    want_after = [after_job(ctx) for ctx in ctxs]
    for ctx in ctxs:
        ctx.close()
    for slicing in ([1] * 9, [4, 4, 1], [1, 8], [9]):
        ctxs = contexts()
        got, got_shards = streamed_sharded(ctxs, SPLIT, inputs, rate, out_fmt, job, slicing)
        got_after = [after_job(ctx) for ctx in ctxs]
        for ctx in ctxs:
            ctx.close()
        what = "slices %s, W = %d" % (slicing, W)
        same_shards(got_shards, want_shards, what)
        assert len(got) == len(want) == nch + 3
        for r in range(nch + 3):
            assert np.array_equal(got[r], want[r]), "output %d, %s" % (r, what)
        for g, (a, b) in enumerate(zip(got_after, want_after)):
            assert a[0] == b[0] and a[1] == b[1], "meters of shard %d, %s" % (g, what)
            same_tuners(a[2], b[2])
            assert a[3] == b[3], "saved state of shard %d, %s" % (g, what)


@pytest.mark.parametrize("W", [1, 4])
def test_sliced_shards_match_the_oracle(oracle, W):
    """the assertions of test_gpu_end_to_end.py::test_batch_run_sharded_over_three_contexts_matches_oracle on the streamed job"""
    case = batch_case(oracle)
    rate, nch, length, ref_out = case.rate, case.nch, case.length, case.ref_out
    for out_fmt, slicing in (("lpcm24", [2, 3, 4]), ("ieee64", [1, 1, 7])):
        ctxs = [case.configured(f, n) for f, n in SPLIT]
        for ctx in ctxs:
            ctx.set_window(W)
        got, shards = streamed_sharded(ctxs, SPLIT, case.inputs, rate, out_fmt, length, slicing)
        lefts, rights, metro = [s[1] for s in shards], [s[2] for s in shards], shards[0][4]
        for r in range(nch + 3):
            want = oracle.wave_encode(out_fmt, ref_out[r])
            assert got[r].size == want.size
            if out_fmt == "ieee64":
                err = rms(got[r].view(np.float64) - ref_out[r])
                assert err <= TOL_RMS, "output %d: RMS %.3e" % (r, err)
            else:
                np.testing.assert_array_equal(got[r], want, err_msg="output %d" % r)
        assert rms(sum(lefts) + metro - ref_out[nch]) <= TOL_RMS and rms(sum(rights) + metro - ref_out[nch + 1]) <= TOL_RMS
        if out_fmt == "lpcm24":
            for g, (ctx, (first, count)) in enumerate(zip(ctxs, SPLIT)):
                lv, pk = ctx.meter_analyze()
                for c in range(count):
                    assert (lv[c], pk[c]) == case.ref_meters[first + c].analyze(), "input meter of channel %d" % (first + c)
                    assert (lv[count + c], pk[count + c]) == case.ref_meters[nch + first + c].analyze(), "output meter of channel %d" % (first + c)
                if g == 0:
                    assert (lv[2 * count], pk[2 * count]) == case.ref_meters[2 * nch].analyze(), "metronome meter"
                    for k in (1, 2):
                        assert (lv[2 * count + k], pk[2 * count + k]) == case.ref_meters[2 * nch + k].analyze(), "master meter %d" % k
            for g, (ctx, (first, count)) in enumerate(zip(ctxs, SPLIT)):
                tuned = ctx.tuner_analyze()
                for c in range(count):
                    want = case.ref_tuners[first + c].analyze()
                    assert tuned[c]["note_index"] == want["note_index"] and tuned[c]["cents"] == want["cents"]
        for ctx in ctxs:
            ctx.close()


def _long_shards(oracle, pkg):
    """_long_job's four channels as 2 + 2: configured(g) = the context of shard g"""
    rate, inputs, _ = _long_job(oracle, pkg)
    from helpers import synth_ir
    from test_gpu_batch_stream import CHAIN
    irs = [synth_ir(2500, seed=70 + c) for c in range(4)]
    split = [(0, 2), (2, 2)]

    def configured(g):
        first, count = split[g]
        ctx = pkg.Context(count, BLOCK)
        for c in range(count):
            for name, p in CHAIN:
                ctx.append_unit(c, name, fir=irs[first + c]) if p == "ir" else ctx.append_unit(c, name, params=p)
        ctx.spatializer_set_sample_rate(rate)
        for c in range(count):
            ctx.spatializer_set_position(c, -60.0 + 40.0 * (first + c), 1.0 + first + c, 0.8)
        ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
        ctx.metronome_configure(4, 150, rate)
        ctx.meter_configure(2 * count + 3)
        ctx.meter_set_enabled(True)
        return ctx
    return rate, inputs, split, configured


def test_a_long_sharded_job_in_random_slicings_has_the_bytes_of_the_one_call_run(oracle):
    """41 blocks, 4 channels as 2 + 2, eight seeded slicings (slices of 1 to 16 blocks, windows of 1 to 16): ONE one-call sharded run is
    the yardstick for all (window sizes change the time blocking, never a sample)."""
    pkg = package()
    rate, inputs, split, configured = _long_shards(oracle, pkg)
    ctxs = [configured(g) for g in range(2)]
    for ctx in ctxs:
        ctx.set_window(4)
    job = max(ctx.batch_length(inputs[f:f + n], rate) for ctx, (f, n) in zip(ctxs, split))
    assert job == 41 * BLOCK
    want, _ = one_call_sharded(ctxs, split, inputs, rate, "lpcm24", job)
    want_after = [after_job(ctx) for ctx in ctxs]
    for ctx in ctxs:
        ctx.close()
    for seed in range(8):
        rng = np.random.default_rng(5200 + seed)
        W = int(rng.choice([1, 2, 4, 8, 16]))
        slicing = random_slicing(rng, 41)
        ctxs = [configured(g) for g in range(2)]
        for ctx in ctxs:
            ctx.set_window(W)
        got, _ = streamed_sharded(ctxs, split, inputs, rate, "lpcm24", job, slicing)
        got_after = [after_job(ctx) for ctx in ctxs]
        for ctx in ctxs:
            ctx.close()
        for r in range(len(want)):
            assert np.array_equal(got[r], want[r]), "seed %d: output %d, W = %d, slices %s" % (seed, r, W, slicing)
        for a, b in zip(got_after, want_after):
            assert a[0] == b[0] and a[1] == b[1], (seed, W, slicing)
            same_tuners(a[2], b[2])


# ---- the finish alone ---------------------------------------------------------------------------------------------------------------
def seq_sum(rows, aux):
    """((p_0 + p_1) + ... + p_{G-1}) + aux in float64, the order of the device"""
    acc = rows[0].copy()
    for p in rows[1:]:
        acc = acc + p
    return acc + aux if aux is not None else acc


def partials(rng, G, n, with_aux):
    """G partial rows of one side and the targets that were planted: ordinary samples, samples beyond +-1, exact +-1, zeros, and sums
    that land EXACTLY on a truncation boundary of an encoder (k / 127, k / 32767.5, k / 8388607.5) although no partial lies on one"""
    rows = [rng.uniform(-0.45, 0.45, n) for _ in range(G)]
    aux = rng.uniform(-0.3, 0.3, n) if with_aux else None
    rows[0][0:64] *= 9.0                                              # beyond +-1 after the sum
    rows[G - 1][64:96] = 7.5
    rows[0][96:128] = -7.5
    for r in rows:
        r[128:256] = 0.0                                              # zeros (with aux: the aux alone)
    if aux is not None:
        aux[192:256] = 0.0
    # planted sums: the last partial closes the gap; kept where float64 makes the sum exact (one ulp of help at most)
    targets = np.concatenate([[1.0, -1.0] * 32, rng.integers(-127, 128, 192) / 127.0, rng.integers(-32767, 32768, 192) / 32767.5,
                              rng.integers(-8388607, 8388608, 192) / 8388607.5])
    at = 256 + np.arange(targets.size)
    assert at[-1] < n
    head = seq_sum([r[at] for r in rows[:-1]], None) if G > 1 else None
    a = aux[at] if aux is not None else 0.0
    best = (targets - a) - (head if head is not None else 0.0)
    exact = np.zeros(targets.size, dtype=bool)
    for cand in (best, np.nextafter(best, np.inf), np.nextafter(best, -np.inf)):
        s = (head + cand if head is not None else cand)
        s = s + a if aux is not None else s
        take = ~exact & (s == targets)
        rows[G - 1][at[take]] = cand[take]
        exact |= take
    rows[G - 1][at[~exact]] = best[~exact]
    kinds = np.repeat([0, 1, 2, 3], [64, 192, 192, 192])
    for kind in range(4):
        assert np.count_nonzero(exact & (kinds == kind)) >= 24, "too few planted sums of kind %d came out exact" % kind
    assert np.array_equal(seq_sum([r[at] for r in rows], a if aux is not None else None)[exact], targets[exact])
    if G > 1:
        on_boundary = lambda v: np.isin(v * 127.0, np.arange(-127, 128)) & (v != 0)
        assert not on_boundary(rows[G - 1][at[(kinds == 1) & exact]]).all()      # the partials themselves are not on the boundary
    return rows, aux


def finish_case(G, fmt, with_aux, blocks, seed):
    rng = np.random.default_rng(seed)
    n = blocks * BLOCK
    lefts, aux = partials(rng, G, n, with_aux)
    rights, _ = partials(rng, G, n, False)
    if aux is not None:                                              # the right side shares the aux row: plant nothing there, shift the special ranges
        rights = [np.roll(r, 4096) for r in rights]
    return lefts, rights, aux


COMBOS = [(G, fmt, aux) for G in (1, 2, 3, 8, 17) for fmt in FORMATS for aux in (False, True)]


def blocks_of(i):
    return 1 + (7 * i + 3) % 20                                      # 1 .. 20, every count taken at least twice over the 60 combinations


def test_the_block_counts_of_the_finish_cases_cover_1_to_20():
    assert sorted(set(blocks_of(i) for i in range(len(COMBOS)))) == list(range(1, 21))


def yardstick(oracle, fmt, lefts, rights, aux):
    """What a finish must give, made without the code under test: the float64 sums of both sides in the documented order (numpy: IEEE adds of
    the same operands in the same order give the same bits) and their bytes from the oracle's encoder, to which tests/test_gpu_io.py pins
    the device's"""
    sums = [seq_sum(lefts, aux), seq_sum(rights, aux)]
    return sums, [oracle.wave_encode(fmt, s) for s in sums]


def finish_against_the_yardstick(finish, fmt, lefts, rights, aux, sums, want, rate=48000):
    """`finish` (the name of an entry point) on fresh contexts: the bytes without and with meters, the master ports' meters against a third,
    identically configured context that is fed the numpy sums block by block (the last block with its true length), and the render report
    against block_stats of the numpy sums.  Returns the bytes and the two contexts' meter readings of the master ports."""
    pkg = package()
    n, wo, what = lefts[0].size, pkg_width(fmt), "%s, G = %d, %s, aux %s, %d samples" % (finish, len(lefts), fmt, aux is not None, lefts[0].size)
    plain = pkg.Context(1, BLOCK)
    got = getattr(plain, finish)(fmt, lefts, rights, aux=aux)
    plain.close()
    for side in range(2):
        assert got[side].size == want[side].size == n * wo, what
        assert np.array_equal(got[side], want[side]), "%s side, %s: %d samples differ" % (
            ("left", "right")[side], what, np.count_nonzero((got[side] != want[side]).reshape(-1, wo).any(axis=1)))
    ctx, third = pkg.Context(1, BLOCK), pkg.Context(1, BLOCK)
    for c in (ctx, third):
        c.meter_configure(5)
        c.meter_set_enabled(True)
    ctx.batch_report_enable()
    got_m = getattr(ctx, finish)(fmt, lefts, rights, aux=aux, sample_rate=rate, run_meters=True)
    for side in range(2):
        assert np.array_equal(got_m[side], want[side]), what
    rep = ctx.batch_report()
    assert rep.shape == (2, -(-n // BLOCK)), what
    assert rep.tobytes() == ctx.block_stats(sums, BLOCK).tobytes(), "the render report, " + what
    for o in range(0, n, BLOCK):
        rows = np.zeros((5, min(BLOCK, n - o)))
        rows[3], rows[4] = sums[0][o:o + BLOCK], sums[1][o:o + BLOCK]
        third.meter_process(rows, rate)
    readings = []
    for c in (ctx, third):
        level, peak = c.meter_analyze()
        readings.append((list(level[3:]), list(peak[3:]), c.meter_state(3), c.meter_state(4)))
    assert readings[0] == readings[1], "the master ports' meters, " + what
    assert ctx.meter_state(3)[1] > 0 and ctx.meter_state(2)[1] == 0  # the master ports were fed, the others were not
    ctx.close()
    third.close()
    return got, readings[0]


@pytest.mark.parametrize("i", range(len(COMBOS)), ids=["G%d-%s-%s" % (G, fmt, "aux" if aux else "noaux") for G, fmt, aux in COMBOS])
def test_finish_master_slice_has_the_bytes_of_finish_master(oracle, i):
    """both entry points run one engine, so each is held against the yardstick; their comparison with each other stays beside it"""
    G, fmt, with_aux = COMBOS[i]
    blocks = blocks_of(i)
    lefts, rights, aux = finish_case(G, fmt, with_aux, blocks, 9000 + i)
    sums, expect = yardstick(oracle, fmt, lefts, rights, aux)
    want, want_meters = finish_against_the_yardstick("batch_finish_master", fmt, lefts, rights, aux, sums, expect)
    got, got_meters = finish_against_the_yardstick("batch_finish_master_slice", fmt, lefts, rights, aux, sums, expect)
    wo = pkg_width(fmt)
    for side in range(2):
        assert got[side].size == want[side].size == blocks * BLOCK * wo
        assert np.array_equal(got[side], want[side]), "%s side, G = %d, %s, aux %s, %d blocks: %d samples differ" % (
            ("left", "right")[side], G, fmt, with_aux, blocks, np.count_nonzero((got[side] != want[side]).reshape(-1, wo).any(axis=1)))
    assert got_meters == want_meters


# ragged lengths: no whole number of blocks, no multiple of 4.  With G = 17 a piece of the finish is 3 blocks, so the longest crosses two piece
# boundaries and ends in a piece of 5 samples; with G = 1 every length is one piece.
RAGGED_SHAPES = [(n, G) for n in (1, 3, 4, 5, 8191, 8193, 7 * BLOCK + 5) for G in (1, 17)]
RAGGED = [(n, G, FORMATS[(3 * j + k) % 6], (j + k) % 2 == 0) for j, (n, G) in enumerate(RAGGED_SHAPES) for k in range(3)]


def test_the_ragged_cases_cover_every_format_and_both_aux_forms_of_every_shape():
    assert set(fmt for _, _, fmt, _ in RAGGED) == set(FORMATS)
    for n, G in RAGGED_SHAPES:
        assert set(aux for m, g, _, aux in RAGGED if (m, g) == (n, G)) == {False, True}


def ragged_case(G, n, with_aux, seed):
    """partials() of n samples; a length too short for what it plants takes the head of a longer case (samples beyond +-1 among them)
    and, in its last sample, a sum far outside +-1 on both sides: the zeros behind a row's end cannot pass for the row's tail"""
    rng = np.random.default_rng(seed)
    m = max(n, 2048)
    lefts, aux = partials(rng, G, m, with_aux)
    rights, _ = partials(rng, G, m, False)
    if aux is not None:                                              # as in finish_case
        rights = [np.roll(r, m // 2) for r in rights]
    lefts, rights = [r[:n].copy() for r in lefts], [r[:n].copy() for r in rights]
    aux = aux[:n].copy() if aux is not None else None
    if n < 4096:
        for rows, v in ((lefts, 7.5), (rights, -7.5)):
            for r in rows:
                r[n - 1] = 0.0
            rows[0][n - 1] = v                                       # the aux is within +-0.3
    return lefts, rights, aux


@pytest.mark.parametrize("i", range(len(RAGGED)), ids=["%d-G%d-%s-%s" % (n, G, fmt, "aux" if aux else "noaux") for n, G, fmt, aux in RAGGED])
def test_finish_master_of_a_ragged_length(oracle, i):
    n, G, fmt, with_aux = RAGGED[i]
    lefts, rights, aux = ragged_case(G, n, with_aux, 9500 + i)
    sums, expect = yardstick(oracle, fmt, lefts, rights, aux)
    if n < 4096:
        assert abs(sums[0][-1]) > 7 and abs(sums[1][-1]) > 7
    finish_against_the_yardstick("batch_finish_master", fmt, lefts, rights, aux, sums, expect)


@pytest.mark.parametrize("G,fmt", [(3, "lpcm24"), (8, "lpcm16"), (17, "ieee32"), (2, "ieee64")])
def test_a_job_finished_in_random_slices_has_the_one_call_finish(G, fmt):
    pkg = package()
    blocks, rate = 37, 44100
    lefts, rights, aux = finish_case(G, fmt, True, blocks, 9900 + G)
    a, b = pkg.Context(1, BLOCK), pkg.Context(1, BLOCK)
    for ctx in (a, b):
        ctx.meter_configure(2)
        ctx.meter_set_enabled(True)
    want = a.batch_finish_master(fmt, lefts, rights, aux=aux, sample_rate=rate, run_meters=True)
    got, at = [], 0
    for k in random_slicing(np.random.default_rng(31 + G), blocks, most=12):
        sl = slice(at * BLOCK, (at + k) * BLOCK)
        got.append(b.batch_finish_master_slice(fmt, [p[sl] for p in lefts], [p[sl] for p in rights], aux=aux[sl], sample_rate=rate, run_meters=True))
        at += k
    for side in range(2):
        assert np.array_equal(np.concatenate([g[side] for g in got]), want[side]), side
    assert [list(v) for v in a.meter_analyze()] == [list(v) for v in b.meter_analyze()]
    for port in (0, 1):
        assert a.meter_state(port) == b.meter_state(port)
    a.close()
    b.close()


def test_finish_master_slice_refusals():
    pkg = package()
    ctx = pkg.Context(1, BLOCK)
    rows = [np.zeros(BLOCK + 4)]
    with pytest.raises(pkg.GdgError, match="whole blocks") as e:
        ctx.batch_finish_master_slice("lpcm16", rows, rows)
    assert e.value.code == pkg.GDG_ERR_INVALID
    left, right = ctx.batch_finish_master("lpcm16", rows, rows)     # the whole-job entry takes any length
    assert left.size == right.size == (BLOCK + 4) * 2 and not left.any() and not right.any()
    with pytest.raises(pkg.GdgError, match="master meters"):
        ctx.batch_finish_master_slice("lpcm16", [np.zeros(BLOCK)], [np.zeros(BLOCK)], sample_rate=48000, run_meters=True)      # no ports configured
    ctx.close()


# ---- contract and memory ----------------------------------------------------------------------------------------------------------------
def test_contract_of_the_streamed_shard(oracle):
    pkg = package()
    nch, blocks = 3, 6
    rate, inputs, configured = _plain_job(oracle, pkg, nch, blocks)
    metas = [(blocks * BLOCK, "lpcm16", rate)] * nch
    other_rate, other_inputs, _ = _plain_job(oracle, pkg, nch, 2, seed=50)
    slice_in = lambda need: [d[0][2 * f:2 * (f + c)] for d, (f, c) in zip(inputs, need)]
    INVALID = pkg.GDG_ERR_INVALID

    def refused(fn, *a, **k):
        with pytest.raises(pkg.GdgError) as e:
            fn(*a, **k)
        assert e.value.code == INVALID and len(str(e.value)) > len("gdg error -1: "), str(e.value)
        return str(e.value)

    ctx = configured()
    canary = [np.full(BLOCK * 3, 0xAB, dtype=np.uint8) for _ in range(nch)]
    canary3 = [np.full(BLOCK * 3, 0xAB, dtype=np.uint8) for _ in range(nch + 3)]
    intact = lambda: all((c == 0xAB).all() for c in canary + canary3)
    # the open call's refusals: nothing is open afterwards
    assert "metronome_to_master must be 0" in refused(ctx.batch_stream_open_shard, metas, rate, "lpcm24", metronome_to_master=True)
    msg = refused(ctx.batch_stream_open_shard, metas, rate, "lpcm24", job_samples=blocks * BLOCK + 100)
    assert str(blocks * BLOCK + 100) in msg and str(blocks * BLOCK) in msg          # names both numbers
    msg = refused(ctx.batch_stream_open_shard, metas, rate, "lpcm24", job_samples=(blocks - 1) * BLOCK)
    assert str((blocks - 1) * BLOCK) in msg and str(blocks * BLOCK) in msg
    refused(ctx.batch_stream_need, 1)                                # none of them opened a job
    # a job opened WITHOUT the metronome: a slice cannot ask for its track
    assert ctx.batch_stream_open_shard(metas, rate, "lpcm24", job_samples=(blocks + 2) * BLOCK, metronome=False) == (blocks + 2) * BLOCK
    refused(ctx.batch_stream_open_shard, metas, rate, "lpcm24")     # a second open
    refused(ctx.batch_stream_open, metas, rate, "lpcm24")
    need = ctx.batch_stream_need(1)
    for want_m in (True, (True, False), (False, True)):
        refused(ctx.batch_stream_step_shard, 1, slice_in(need), metronome=want_m, outs=canary)
    # master_left missing
    lib, ct = pkg.lib(), __import__("ctypes")
    ins = slice_in(need)
    keep = [np.ascontiguousarray(b) for b in ins]
    in_ptrs = (ct.c_void_p * nch)(*[k.ctypes.data for k in keep])
    out_ptrs = (ct.c_void_p * nch)(*[c.ctypes.data for c in canary])
    right = np.full(BLOCK, 7.0)
    so = pkg.BatchShardOut(None, right.ctypes.data, None, None, 0)
    for slice_arg in (ct.byref(so), None):
        rc = lib.gdg_batch_stream_step_shard(ctx._h, 1, in_ptrs, out_ptrs, slice_arg)
        assert rc == INVALID
        assert "partial master mix" in refused(ctx._check, rc)
    assert (right == 7.0).all()
    # the plain step on a shard's job; the one-call runs and the release while it is open
    ctx._stream_width = 3
    assert "shard" in refused(ctx.batch_stream_step, 1, slice_in(need), canary3)
    refused(ctx.batch_run_shard, other_inputs, rate, "lpcm24")
    refused(ctx.batch_run, other_inputs, rate, "lpcm24", outs=[np.full(2 * BLOCK * 3, 0xAB, dtype=np.uint8) for _ in range(nch + 3)])
    refused(ctx.batch_release)
    refused(ctx.batch_stream_need, blocks + 3)                       # beyond the job's end (the job is blocks + 2 long)
    refused(ctx.batch_stream_step_shard, 1, [None] * nch, outs=canary)      # frames asked for and not brought
    assert intact()
    # ... after all of which the job is still open and runs: 6 blocks of files, 2 of padding
    outs, left, rightp, mb, mf = ctx.batch_stream_step_shard(4, slice_in(ctx.batch_stream_need(4)))
    assert mb is None and mf is None and left.any() and rightp.any()
    ctx.batch_stream_step_shard(4, slice_in(ctx.batch_stream_need(4)))
    refused(ctx.batch_stream_step_shard, 1, [None] * nch, outs=canary)      # after the last block
    ctx.batch_stream_close()
    # the shard's step on a plain job
    assert ctx.batch_stream_open(metas, rate, "lpcm24") == blocks * BLOCK
    need = ctx.batch_stream_need(1)
    assert "not a shard" in refused(ctx.batch_stream_step_shard, 1, slice_in(need), outs=canary)
    assert intact()
    ctx.batch_stream_step(1, slice_in(need))                         # the plain job goes on
    ctx.batch_stream_close()
    ctx.close()

    # a shard's job abandoned after 4 of its 6 blocks: the context goes on as after gdg_batch_run_shard of those 4 blocks
    ctx = configured()
    ctx.set_window(2)
    gen = ctx.batch_stream_shard(inputs, rate, "lpcm24", 1, metronome=True)
    got_head = [next(gen) for _ in range(4)]
    gen.close()                                                      # closes the job
    got = ctx.batch_run_shard(other_inputs, rate, "lpcm24", metronome=True)
    ctx.close()
    ctx = configured()
    ctx.set_window(2)
    want_head = ctx.batch_run_shard([(d[:2 * 4 * BLOCK], f, r) for d, f, r in inputs], rate, "lpcm24", metronome=True)
    want = ctx.batch_run_shard(other_inputs, rate, "lpcm24", metronome=True)
    ctx.close()
    for c in range(nch):
        assert np.array_equal(np.concatenate([p[0][c] for p in got_head]), want_head[0][c]), c
        assert np.array_equal(got[0][c], want[0][c]), c
    for r in range(1, 5):
        assert np.array_equal(np.concatenate([p[r] for p in got_head]), want_head[r]), r
        assert np.array_equal(got[r], want[r]), r


def test_device_memory_of_a_streamed_shard_follows_the_slice_not_the_job(oracle):
    pkg = package()
    nch = 8
    kib = {}
    for blocks in (16, 64):
        rate, inputs, configured = _plain_job(oracle, pkg, nch, blocks)
        inputs = [(d, f, 44100 if c % 2 else r) for c, (d, f, r) in enumerate(inputs)]
        ctx = configured()
        ctx.set_window(4)
        assert ctx.get_option("stat_batch_device_kib") == 0
        seen = []
        for k, part in enumerate(ctx.batch_stream_shard(inputs, rate, "lpcm24", 4, metronome=True)):
            seen.append(ctx.get_option("stat_batch_device_kib"))
        assert len(seen) >= blocks // 4 and seen[0] > 0
        assert all(v == seen[0] for v in seen), "the buffers grew after the first slice: %s" % seen
        kib[blocks] = seen[0]
        length = ctx.batch_length(inputs, rate)
        if blocks == 64:
            assert seen[0] * 1024 < nch * length * 8                 # what the one-call shard allocates for the decoded inputs alone
        ctx.batch_release()
        assert ctx.get_option("stat_batch_device_kib") == 0
        ctx.close()
    assert kib[16] == kib[64], kib
    # which metronome buffers a slice passes does not move the figure either
    rate, inputs, configured = _plain_job(oracle, pkg, nch, 8)
    ctx = configured()
    ctx.set_window(4)
    metas = [(8 * BLOCK, "lpcm16", rate)] * nch
    ctx.batch_stream_open_shard(metas, rate, "lpcm24", metronome=True)
    seen = []
    for want_m in (False, True, (True, False), (False, True)):
        need = ctx.batch_stream_need(2)
        ctx.batch_stream_step_shard(2, [d[0][2 * f:2 * (f + c)] for d, (f, c) in zip(inputs, need)], metronome=want_m)
        seen.append(ctx.get_option("stat_batch_device_kib"))
    ctx.batch_stream_close()
    ctx.close()
    assert all(v == seen[0] for v in seen), seen
