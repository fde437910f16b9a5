"""Checkpoint and resume of a streamed batch run (gdg_batch_stream_checkpoint / _resume / _resume_shard, gdg_state_verify).  The yardstick is
always the UNINTERRUPTED streamed run on a fresh, identically configured context: a job cut at a slice boundary, written into a blob,
its context destroyed, and continued in a new context writes the same bytes -- every container format -- and ends in the same meters,
tuner results and saved state.  The digest's yardstick is the plain-Python restatement in tests/test_checkpoint_abi.py."""
import ctypes as C
import struct

import numpy as np
import pytest

from helpers import package
from test_checkpoint_abi import digest
from test_gpu_batch_stream import BLOCK, FORMATS, _long_job, batch_case, random_slicing
from test_gpu_batch_stream_shard import SPLIT, same_shards, streamed_sharded

pytestmark = pytest.mark.gpu

KW = dict(metronome_to_master=True, run_meters=True, tuner_enqueue=True)
KW_SHARD = dict(run_meters=True, tuner_enqueue=True)
HEADER = 48                                       # container header: the payload (and the digest's range) starts here; the digest sits at 32


def split_inputs(ctx, inputs):
    metas, datas, widths = ctx._stream_split(inputs)
    return metas, datas, widths


def feed(ctx, datas, widths, blocks):
    need = ctx.batch_stream_need(blocks)
    return need, [None if d is None or not c else d[f * w:(f + c) * w] for d, w, (f, c) in zip(datas, widths, need)]


def run_slices(ctx, inputs, slicing, at=0, firsts=None):
    """the open job's next slices, the job standing at block `at`; -> list of per-slice output lists.  firsts (a dict) receives, per
    block position a slice starts at, the `first` of every input there"""
    _, datas, widths = split_inputs(ctx, inputs)
    parts = []
    for k in slicing:
        need, ins = feed(ctx, datas, widths, k)
        if firsts is not None:
            firsts[at] = [f for f, _ in need]
        parts.append(ctx.batch_stream_step(k, ins))
        at += k
    return parts


def joined(parts, rows):
    return [np.concatenate([p[r] for p in parts]) if parts else np.zeros(0, dtype=np.uint8) for r in range(rows)]


def after_state(ctx, ports):
    """everything the job leaves behind that a caller can read, bit for bit"""
    meters = [ctx.meter_state(p) for p in range(ports)]
    meters = [(struct.pack("<d", c), struct.pack("<d", p), n) for c, p, n in meters]
    lv, pk = ctx.meter_analyze()
    tuned = [(struct.pack("<d", r.frequency), int(r.note_index), int(r.cents)) for r in ctx.tuner_analyze(raw=True)]
    return meters, ([int(v) for v in lv], [int(v) for v in pk]), tuned, bytes(ctx.save_state())


def slicing_for(rng, blocks):
    """a random slicing whose last slice is one block: the job's last step is then one block in every run that is compared, whatever
    the window (include/gdg.h: a saved state is equal where the job's last steps coincide)"""
    return (random_slicing(rng, blocks - 1, most=4) + [1]) if blocks else []


@pytest.mark.parametrize("W", [1, 4])
@pytest.mark.parametrize("out_fmt", FORMATS)
def test_a_resumed_job_writes_the_bytes_of_the_uninterrupted_one(oracle, out_fmt, W):
    """_batch_case's job (six formats in, two resampled inputs, an empty input, a stereo pick, metronome in the master, meters, tuner) cut
    before the first slice, after the first, inside the tail where all but one input have ended, and after the last slice."""
    pkg = package()
    case = batch_case(oracle)
    rate, nch, inputs, blocks = case.rate, case.nch, case.inputs, case.length // BLOCK
    ports = 2 * nch + 3
    rng = np.random.default_rng(300 + W)
    A = slicing_for(rng, blocks)
    ref = case.configured()
    ref.set_window(W)
    metas, _, _ = split_inputs(ref, inputs)
    assert ref.batch_stream_open(metas, rate, out_fmt, **KW) == case.length
    firsts = {}
    want_parts = run_slices(ref, inputs, A, 0, firsts)
    ref.batch_stream_close()
    want = joined(want_parts, nch + 3)
    want_after = after_state(ref, ports)
    ref.close()
    tail_cut = len(A) - 1                                         # before the last block: only the 44.1 kHz file is still running
    assert tail_cut > 1 and sum(A[:tail_cut]) == blocks - 1
    for cut in (0, 1, tail_cut, len(A)):
        src = case.configured()
        src.set_window(W)
        src.batch_stream_open(metas, rate, out_fmt, **KW)
        head = run_slices(src, inputs, A[:cut])
        blob = src.batch_stream_checkpoint()
        src.close()                                               # gdg_ctx_destroy with the job open: the process is gone
        done = sum(A[:cut]) * BLOCK
        dst = case.configured()
        dst.set_window(W)
        assert dst.batch_stream_resume(metas, rate, out_fmt, blob, **KW) == done
        left = blocks - sum(A[:cut])
        if left:
            assert [f for f, _ in dst.batch_stream_need(1)] == firsts[sum(A[:cut])], "first[i] continues where the job stood (cut %d)" % cut
            B = slicing_for(np.random.default_rng(900 + 10 * W + cut), left)
            tail = run_slices(dst, inputs, B, sum(A[:cut]))
        else:
            tail = []
            for call in (lambda: dst.batch_stream_need(1), lambda: dst.batch_stream_step(1, [None] * nch)):
                with pytest.raises(pkg.GdgError) as e:
                    call()
                assert e.value.code == pkg.GDG_ERR_INVALID and "delivered its last block" in str(e.value)
        dst.batch_stream_close()
        got = joined(head + tail, nch + 3)
        for r in range(nch + 3):
            assert np.array_equal(got[r], want[r]), "output %d, cut after slice %d of %s, W = %d, %s" % (r, cut, A, W, out_fmt)
        got_after = after_state(dst, ports)
        dst.close()
        assert got_after[0] == want_after[0], "meter records, cut %d" % cut
        assert got_after[1] == want_after[1], "meter levels, cut %d" % cut
        assert got_after[2] == want_after[2], "tuner results, cut %d" % cut
        assert got_after[3] == want_after[3], "saved state, cut %d" % cut


def test_a_checkpoint_changes_nothing(oracle):
    """a checkpoint after every slice (and before the first): the same bytes, the same final state, no fewer continued sums"""
    case = batch_case(oracle)
    rate, nch, inputs, blocks = case.rate, case.nch, case.inputs, case.length // BLOCK
    slicing = random_slicing(np.random.default_rng(77), blocks, most=3)
    results = []
    for with_checkpoints in (False, True):
        ctx = case.configured()
        metas, datas, widths = split_inputs(ctx, inputs)
        ctx.batch_stream_open(metas, rate, "ieee64", **KW)
        parts, sizes = [], []
        for k in slicing:
            if with_checkpoints:
                sizes.append(len(ctx.batch_stream_checkpoint()))
            _, ins = feed(ctx, datas, widths, k)
            parts.append(ctx.batch_stream_step(k, ins))
        if with_checkpoints:
            sizes.append(len(ctx.batch_stream_checkpoint()))
            assert sizes[0] < sizes[-1]                          # before the first slice every unit is fresh and no tuner ring exists
        ctx.batch_stream_close()
        results.append((joined(parts, nch + 3), after_state(ctx, 2 * nch + 3), ctx.get_option("stat_premac_launches_used")))
        ctx.close()
    (plain, plain_after, plain_used), (ck, ck_after, ck_used) = results
    for r in range(nch + 3):
        assert np.array_equal(plain[r], ck[r]), "output %d" % r
    assert plain_after == ck_after
    assert ck_used >= plain_used


@pytest.mark.parametrize("windows", [(16, 4, 0), (1, 16, 2), (4, 1, 3)])
def test_resume_under_another_window_and_group_count(oracle, windows):
    """the 41-block job: the target's window and channel groups differ from the source's, the bytes do not"""
    pkg = package()
    w_src, w_dst, groups = windows
    rate, inputs, configured = _long_job(oracle, pkg)
    ref = configured()
    ref.set_window(w_src)
    metas, _, _ = split_inputs(ref, inputs)
    length = ref.batch_stream_open(metas, rate, "lpcm24", **KW)
    blocks = length // BLOCK
    rng = np.random.default_rng(500 + w_src)
    A = random_slicing(rng, blocks)
    want = joined(run_slices(ref, inputs, A), len(inputs) + 3)
    ref.close()
    for cut in (1, len(A) // 2):
        src = configured()
        src.set_window(w_src)
        src.batch_stream_open(metas, rate, "lpcm24", **KW)
        head = run_slices(src, inputs, A[:cut])
        blob = src.batch_stream_checkpoint()
        src.close()
        dst = configured()
        dst.set_window(w_dst)
        dst.set_overlap(groups)
        assert dst.batch_stream_resume(metas, rate, "lpcm24", blob, **KW) == sum(A[:cut]) * BLOCK
        B = random_slicing(np.random.default_rng(600 + cut), blocks - sum(A[:cut]))
        tail = run_slices(dst, inputs, B)
        dst.close()
        got = joined(head + tail, len(inputs) + 3)
        for r in range(len(want)):
            assert np.array_equal(got[r], want[r]), "output %d, window %d -> %d, cut after slice %d of %s" % (r, w_src, w_dst, cut, A)


def shard_slices(ctxs, inputs, out_fmt, slicing, finish_on=0):
    """the next slices of three open shard jobs, each slice's master finished; -> [(parts per shard, (left, right))]"""
    rate = 48000
    split = [ctx._stream_split(inputs[f:f + n]) for ctx, (f, n) in zip(ctxs, SPLIT)]
    out = []
    for k in slicing:
        parts = []
        for g, (ctx, (_, datas, widths)) in enumerate(zip(ctxs, split)):
            _, ins = feed(ctx, datas, widths, k)
            parts.append(ctx.batch_stream_step_shard(k, ins, metronome=(g == 0)))
        master = ctxs[finish_on].batch_finish_master_slice(out_fmt, [p[1] for p in parts], [p[2] for p in parts], aux=parts[0][4], sample_rate=rate,
                                                           run_meters=True)
        out.append((parts, master))
    return out


@pytest.mark.parametrize("out_fmt", ["lpcm24", "ieee64"])
def test_a_sharded_job_resumes_in_three_new_contexts(oracle, out_fmt):
    pkg = package()
    case = batch_case(oracle)
    rate, nch, inputs, job = case.rate, case.nch, case.inputs, case.length
    slicing = [2, 3, 1, 3]
    ctxs = [case.configured(f, n) for f, n in SPLIT]
    want, want_shards = streamed_sharded(ctxs, SPLIT, inputs, rate, out_fmt, job, slicing)
    want_after = [after_state(ctx, 2 * n + 3) for ctx, (_, n) in zip(ctxs, SPLIT)]
    for ctx in ctxs:
        ctx.close()

    def metas_of(ctx, f, n):
        return ctx._stream_split(inputs[f:f + n])[0]

    for cut in (1, 3):
        src = [case.configured(f, n) for f, n in SPLIT]
        for g, (ctx, (f, n)) in enumerate(zip(src, SPLIT)):
            assert ctx.batch_stream_open_shard(metas_of(ctx, f, n), rate, out_fmt, job_samples=job, metronome=(g == 0), **KW_SHARD) == job
        head = shard_slices(src, inputs, out_fmt, slicing[:cut])
        blobs = [ctx.batch_stream_checkpoint() for ctx in src]
        for ctx in src:
            ctx.close()
        dst = [case.configured(f, n) for f, n in SPLIT]
        for g, (ctx, (f, n)) in enumerate(zip(dst, SPLIT)):
            done = ctx.batch_stream_resume_shard(metas_of(ctx, f, n), rate, out_fmt, blobs[g], job_samples=job, metronome=(g == 0), **KW_SHARD)
            assert done == sum(slicing[:cut]) * BLOCK
        rest = [1] * (job // BLOCK - sum(slicing[:cut]))           # another slicing, every shard alike
        tail = shard_slices(dst, inputs, out_fmt, rest)
        for ctx in dst:
            ctx.batch_stream_close()
        slices = head + tail
        shards = []
        for g in range(3):
            outs = [np.concatenate([s[0][g][0][c] for s in slices]) for c in range(SPLIT[g][1])]
            row = lambda r: None if slices[0][0][g][r] is None else np.concatenate([s[0][g][r] for s in slices])
            shards.append((outs, row(1), row(2), row(3), row(4)))
        ml, mr = np.concatenate([s[1][0] for s in slices]), np.concatenate([s[1][1] for s in slices])
        got = sum((s[0] for s in shards), []) + [ml, mr, shards[0][3]]
        same_shards(shards, want_shards, "cut after slice %d" % cut)
        for r in range(nch + 3):
            assert np.array_equal(got[r], want[r]), "output %d, cut after slice %d" % (r, cut)
        got_after = [after_state(ctx, 2 * n + 3) for ctx, (_, n) in zip(dst, SPLIT)]
        for ctx in dst:
            ctx.close()
        for g in range(3):
            assert got_after[g][:3] == want_after[g][:3], "meters and tuner of shard %d, cut %d" % (g, cut)
            assert got_after[g][3] == want_after[g][3], "saved state of shard %d, cut %d" % (g, cut)

    # a shard's blob is no plain job's and the other way round: refused, nothing written, no job open
    f, n = SPLIT[0]
    ctx = case.configured(f, n)
    metas = metas_of(ctx, f, n)
    ctx.batch_stream_open(metas, rate, out_fmt, run_meters=True, tuner_enqueue=True)
    plain_blob = ctx.batch_stream_checkpoint()
    ctx.batch_stream_close()
    ctx.batch_run(inputs[f:f + n], rate, out_fmt, run_meters=True, tuner_enqueue=True)       # a target that holds state
    before = after_state(ctx, 2 * n + 3)
    for call, word in ((lambda: ctx.batch_stream_resume(metas, rate, out_fmt, blobs[0], **KW_SHARD), "shard"),
                       (lambda: ctx.batch_stream_resume_shard(metas, rate, out_fmt, plain_blob, job_samples=job, metronome=True, **KW_SHARD), "plain")):
        with pytest.raises(pkg.GdgError) as e:
            call()
        assert e.value.code == pkg.GDG_ERR_INVALID and word in str(e.value), str(e.value)
        with pytest.raises(pkg.GdgError) as e:
            ctx.batch_stream_need(1)
        assert "no streamed batch run is open" in str(e.value)
        assert after_state(ctx, 2 * n + 3) == before
    ctx.close()


def test_a_refused_resume_writes_nothing(oracle):
    pkg = package()
    case = batch_case(oracle)
    rate, nch, inputs = case.rate, case.nch, case.inputs
    ports = 2 * nch + 3
    src = case.configured()
    metas, _, _ = split_inputs(src, inputs)
    src.batch_stream_open(metas, rate, "lpcm24", **KW)
    run_slices(src, inputs, [2, 1])
    blob = src.batch_stream_checkpoint()
    src.close()
    flipped = bytearray(blob)
    flipped[len(blob) - 1000] ^= 0x04                               # deep inside the payload: only the digest can see it
    shorter = list(metas)
    shorter[1] = (metas[1][0] - 1,) + tuple(metas[1][1:])

    def target(meter_ports=ports, swap_unit=False, meters=True):
        ctx = case.configured()
        if swap_unit:                                             # channel 2: a flanger where the job has its chorus
            chain = list(ctx._chains[2])
            chain[3] = (ctx.unit_create(2, "flanger"), False)
            ctx.chain_set(2, [h for h, _ in chain], [b for _, b in chain])
        if meter_ports != ports:
            ctx.meter_configure(meter_ports)
            ctx.meter_set_enabled(True)
        ctx.batch_run(inputs, rate, "lpcm24", metronome_to_master=True, run_meters=meters, tuner_enqueue=True)      # non-trivial state everywhere
        if not meters:
            ctx.meter_process(np.random.default_rng(5).uniform(-0.5, 0.5, (meter_ports, 4096)), rate)
        return ctx

    def refused(ctx, n_ports, word, *args, **kw):
        before = after_state(ctx, n_ports)
        with pytest.raises(pkg.GdgError) as e:
            ctx.batch_stream_resume(*args, **kw)
        assert e.value.code == pkg.GDG_ERR_INVALID and word in str(e.value), "%r not named in: %s" % (word, e.value)
        with pytest.raises(pkg.GdgError) as e:
            ctx.batch_stream_need(1)
        assert "no streamed batch run is open" in str(e.value)
        assert after_state(ctx, n_ports) == before, "a refused resume (%s) changed the target" % word

    ctx = target()
    refused(ctx, ports, "truncated", metas, rate, "lpcm24", blob[:len(blob) // 2], **KW)
    refused(ctx, ports, "truncated", metas, rate, "lpcm24", blob[:40], **KW)
    refused(ctx, ports, "digest", metas, rate, "lpcm24", bytes(flipped), **KW)
    refused(ctx, ports, "samples_per_channel", shorter, rate, "lpcm24", blob, **KW)
    refused(ctx, ports, "out_format", metas, rate, "lpcm16", blob, **KW)
    # ... and the same target takes the intact blob afterwards
    assert ctx.batch_stream_resume(metas, rate, "lpcm24", blob, **KW) == 3 * BLOCK
    ctx.close()
    ctx = target(meter_ports=ports - 1, meters=False)
    refused(ctx, ports - 1, "ports", metas, rate, "lpcm24", blob, **KW)
    # without meters in the job the blob's own port count is what does not fit
    src = case.configured()
    src.batch_stream_open(metas, rate, "lpcm24", tuner_enqueue=True)
    run_slices(src, inputs, [1])
    blob_no_meters = src.batch_stream_checkpoint()
    src.close()
    refused(ctx, ports - 1, "meter ports", metas, rate, "lpcm24", blob_no_meters, tuner_enqueue=True)
    ctx.close()
    ctx = target(swap_unit=True)
    refused(ctx, ports, "unit type", metas, rate, "lpcm24", blob, **KW)
    ctx.close()


def test_the_digest_is_the_restated_function_and_verify_checks_it(oracle):
    pkg = package()
    case = batch_case(oracle)
    rate, inputs = case.rate, case.inputs
    ctx = case.configured()
    metas, _, _ = split_inputs(ctx, inputs)
    # no job open: nothing to checkpoint
    for call in (ctx.batch_stream_checkpoint,):
        with pytest.raises(pkg.GdgError) as e:
            call()
        assert e.value.code == pkg.GDG_ERR_INVALID
    ctx.batch_stream_open(metas, rate, "ieee32", **KW)
    fresh = ctx.batch_stream_checkpoint()                          # before the first slice: a small container
    run_slices(ctx, inputs, [3])
    blob = ctx.batch_stream_checkpoint()
    # into less capacity: refused, the size needed reported
    size, written = C.c_size_t(0), C.c_size_t(0)
    assert pkg.lib().gdg_batch_stream_checkpoint_size(ctx._h, C.byref(size)) == pkg.GDG_OK and size.value == len(blob)
    small = C.create_string_buffer(size.value - 16)
    assert pkg.lib().gdg_batch_stream_checkpoint(ctx._h, small, size.value - 16, C.byref(written)) == pkg.GDG_ERR_INVALID
    assert written.value == len(blob) and not any(small.raw[:64])
    ctx.batch_stream_close()
    for b in (fresh, blob):
        assert b[:8] == b"GDGCKPT\0" and struct.unpack_from("<IIQ", b, 8) == (1, HEADER, len(b)) and len(b) % 16 == 0
        assert b[32:48] == digest(b[HEADER:]), "the container's digest is the restated function of its payload"
        assert b[32:48] == pkg.checkpoint_digest(b[HEADER:])
        ctx.state_verify(b)
    assert fresh[32:48] != blob[32:48]
    for at in (HEADER, HEADER + 200, len(blob) // 2, len(blob) - 1):
        bad = bytearray(blob)
        bad[at] ^= 0x80
        with pytest.raises(pkg.GdgError) as e:
            ctx.state_verify(bytes(bad))
        assert e.value.code == pkg.GDG_ERR_INVALID and "digest" in str(e.value), (at, str(e.value))
    # two granules swapped: the same bytes in another order
    bad = bytearray(blob)
    a, b = len(blob) - 64, len(blob) - 32
    if bad[a:a + 16] == bad[b:b + 16]:
        bad[a] ^= 1
        bad[32:48] = digest(bytes(bad[HEADER:]))
        ctx.state_verify(bytes(bad))
    bad[a:a + 16], bad[b:b + 16] = bad[b:b + 16], bad[a:a + 16]
    with pytest.raises(pkg.GdgError) as e:
        ctx.state_verify(bytes(bad))
    assert "digest" in str(e.value)
    # a bare version-1 state blob has no digest
    with pytest.raises(pkg.GdgError) as e:
        ctx.state_verify(ctx.save_state())
    assert e.value.code == pkg.GDG_ERR_INVALID and "no digest" in str(e.value)
    ctx.close()
