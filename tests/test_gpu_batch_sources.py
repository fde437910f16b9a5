"""Shared sources of a batch job (include/gdg.h, gdg_batch_set_sources): a source map makes a channel read another channel's input entry,
which is then gathered, uploaded, decoded and resampled once and stored to every row that reads it.

The specification of every bit is the SAME job without a map, every reader's entry a copy of its root's: each test builds two contexts
with the same chains -- one with the map and the readers' entries left empty (None / NULL), one without a map and with duplicated
entries -- and compares with == on bytes: the N + 3 files, meter records and readings, tuner results, the render report and the
gdg_state_save blob.  No tolerance appears anywhere.

The core job: 6 channels at 48 kHz with six different chains (no two outputs agree); source A 16-bit mono at 48 kHz, 20 000 frames (not
a block multiple); source B 24-bit stereo of which channel 1 is taken, 44.1 kHz, 17 003 frames (resampled, strided, odd); map
[0, 0, 2, 0, 2, 5]: fans of 3, 2 and 1, channel 5 an empty input of its own.  The job has three blocks, so window 2 steps 2 + 1."""
import struct

import numpy as np
import pytest

from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
RATE = 48000
NCH = 6
MAP = [0, 0, 2, 0, 2, 5]
KW = dict(metronome_to_master=True, run_meters=True, tuner_enqueue=True)
KW_SHARD = dict(run_meters=True, tuner_enqueue=True)
FORMATS = ["lpcm8", "lpcm16", "lpcm24", "lpcm32", "ieee32", "ieee64"]
OUT = "lpcm24"


def file_bytes(fmt, frames, channels, seed, rate):
    """the data section of a file: interleaved frames of `channels` different signals, quantised here (any code is a valid sample)"""
    x = np.stack([0.6 * synth_signal(seed + 7 * k, frames, rate) for k in range(channels)], axis=1).reshape(-1)
    if fmt == "lpcm8":
        return np.clip(np.round(127.0 * x) + 128, 0, 255).astype(np.uint8)
    if fmt == "lpcm16":
        return np.round(32767.0 * x).astype("<i2").view(np.uint8)
    if fmt == "lpcm24":
        return np.ascontiguousarray(np.round(8388607.0 * x).astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)
    if fmt == "lpcm32":
        return np.round(2147483647.0 * x).astype("<i4").view(np.uint8)
    return x.astype("<f4" if fmt == "ieee32" else "<f8").view(np.uint8)


def source_a(fmt="lpcm16", frames=20000):
    return (file_bytes(fmt, frames, 1, 1, RATE), fmt, RATE)


def source_b():
    return (file_bytes("lpcm24", 17003, 2, 2, 44100), "lpcm24", 44100, 2, 1)


def core_inputs(a=None, b=None):
    """(with the map: readers' entries empty, without: copies)"""
    a, b = a or source_a(), b or source_b()
    return [a, None, b, None, None, None], [a, a, b, a, b, None]


POSITIONS = [(-60.0 + 25.0 * c, 0.8 + 0.4 * c, 0.9 - 0.1 * c) for c in range(NCH)]
TICK, TOCK = 0.3 * np.sin(np.arange(700) * 0.21), 0.25 * np.sin(np.arange(450) * 0.33)


def set_chain(ctx, local, channel):
    """six different short chains, by the JOB's channel number"""
    kind = channel % NCH
    if kind == 0:
        ctx.append_unit(local, "distortion")
    elif kind == 1:
        ctx.append_unit(local, "tone_stack")
    elif kind == 2:
        ctx.append_unit(local, "power_amp", fir=synth_ir(300, seed=77))
    elif kind == 3:
        ctx.append_unit(local, "reverb", params=[30])
    elif kind == 4:
        ctx.append_unit(local, "overdrive", params=[0, 20, 100, 0, 1, 1])      # 2 x oversampled
    # kind 5: an empty chain


def configured(first=0, count=NCH, window=1, chains=True):
    pkg = package()
    ctx = pkg.Context(count, BLOCK)
    for c in range(count):
        if chains:
            set_chain(ctx, c, first + c)
    ctx.spatializer_set_sample_rate(RATE)
    for c in range(count):
        ctx.spatializer_set_position(c, *POSITIONS[(first + c) % NCH])
    ctx.metronome_set_sounds(TICK, TOCK)
    ctx.metronome_configure(3, 200, RATE)
    ctx.meter_configure(2 * count + 3)
    ctx.meter_set_enabled(True)
    ctx.set_window(window)
    ctx.batch_report_enable()
    return ctx


def after(ctx, ports):
    """everything a job leaves behind that a caller can read, bit for bit"""
    meters = [ctx.meter_state(p) for p in range(ports)]
    meters = [(struct.pack("<d", c), struct.pack("<d", p), n) for c, p, n in meters]
    lv, pk = ctx.meter_analyze()
    tuned = [(struct.pack("<d", r.frequency), int(r.note_index), int(r.cents)) for r in ctx.tuner_analyze(raw=True)]
    return dict(meters=meters, readings=([int(v) for v in lv], [int(v) for v in pk]), tuner=tuned, state=bytes(ctx.save_state()))


def one_call(inputs, source, window=1, count=NCH, chains=True):
    """-> (output bytes, what is left behind, report bytes, the two counters)"""
    ctx = configured(0, count, window, chains)
    if source is not None:
        ctx.batch_set_sources(source)
    outs = ctx.batch_run(inputs, RATE, OUT, **KW)
    res = ([o.tobytes() for o in outs], after(ctx, 2 * count + 3), ctx.batch_report().tobytes(),
           (ctx.get_option("stat_batch_upload_bytes"), ctx.get_option("stat_batch_resampled_samples")))
    ctx.close()
    return res


def same(got, want, what):
    assert len(got[0]) == len(want[0])
    for r, (g, w) in enumerate(zip(got[0], want[0])):
        assert g == w, "%s: output file %d" % (what, r)
    for key in ("meters", "readings", "tuner", "state"):
        assert got[1][key] == want[1][key], "%s: %s" % (what, key)
    assert got[2] == want[2], "%s: render report" % what


_cache = {}


def duplicated(window):
    """the specification: the core job without a map, entries copied; computed once per window and left unchanged"""
    if window not in _cache:
        _cache[window] = one_call(core_inputs()[1], None, window)
    return _cache[window]


def covered_bytes(inp):
    """the file bytes of one input that the job covers: every source frame its output samples read (gdg_batch_stream_span)"""
    pkg = package()
    data, fmt, rate = inp[0], inp[1], inp[2]
    channels = inp[3] if len(inp) > 3 else 1
    width = pkg.lib().gdg_wave_bytes_per_sample(pkg.WAVE_FORMATS[fmt]) * channels
    frames = data.size // width
    n_out = frames if rate == RATE else pkg.lib().gdg_resample_time_length(frames, rate, RATE)
    first, count = pkg.batch_stream_span(frames, rate, RATE, 0, n_out)
    return (first + count) * width, n_out


# ---- the core job --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 2])
def test_core_job_equals_the_duplicated_run(window):
    mapped, _ = core_inputs()
    want = duplicated(window)
    got = one_call(mapped, MAP, window)
    same(got, want, "window %d" % window)
    assert len(set(want[0][:NCH])) == NCH, "no two chain outputs agree"
    assert len(want[0][0]) == 3 * BLOCK * 3, "20 000 frames: three blocks of 24-bit samples"


def test_counters_upload_and_resample_once_per_root():
    mapped, dup = core_inputs()
    got, want = one_call(mapped, MAP), duplicated(1)
    a_bytes, _ = covered_bytes(mapped[0])
    b_bytes, b_out = covered_bytes(mapped[2])
    assert a_bytes == 20000 * 2 and b_bytes == 17003 * 6 and b_out == 18506
    assert got[3] == (a_bytes + b_bytes, b_out), "the roots' file bytes once; B's output samples once"
    assert want[3] == (3 * a_bytes + 2 * b_bytes, 2 * b_out), "the duplicated run: per channel"
    assert got[3][0] < want[3][0]


# ---- formats -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_through_the_fans(fmt):
    """source A in each of the six formats; the 8-bit and the 24-bit file have an odd frame count, so their pieces end off a word and the
    byte-wise tail runs beside the word-wise path; B keeps the strided path.  Fans of 3 (A), 2 (B) and 1 (the empty channel's own)."""
    frames = {"lpcm8": 20001, "lpcm24": 19999}.get(fmt, 20000)
    a = source_a(fmt, frames)
    mapped, dup = core_inputs(a=a)
    same(one_call(mapped, MAP, 2), one_call(dup, None, 2), fmt)


# ---- the streamed job ----------------------------------------------------------------------------------------------------------------
def streamed(inputs, source, slicing, window=1, null_readers=False):
    ctx = configured(0, NCH, window)
    if source is not None:
        ctx.batch_set_sources(source)
    metas, datas, widths = ctx._stream_split(inputs)
    assert ctx.batch_stream_open(metas, RATE, OUT, **KW) == 3 * BLOCK
    parts, reps, needs = [], [], []
    for k in slicing:
        need = ctx.batch_stream_need(k)
        needs.append(need)
        ins = [None if d is None or not c else d[f * w:(f + c) * w] for d, w, (f, c) in zip(datas, widths, need)]
        if null_readers:
            assert all(ins[c] is None for c in range(NCH) if source[c] != c), "a reader hands nothing over"
        parts.append(ctx.batch_stream_step(k, ins))
        reps.append(ctx.batch_report())
    ctx.batch_stream_close()
    outs = [b"".join(p[r].tobytes() for p in parts) for r in range(NCH + 3)]
    res = (outs, after(ctx, 2 * NCH + 3), np.concatenate(reps, axis=1).tobytes(), None)
    ctx.close()
    return res, needs


@pytest.mark.parametrize("slicing", [(1, 2), (1, 1, 1)])
def test_streamed_job(slicing):
    mapped, dup = core_inputs()
    got, needs = streamed(mapped, MAP, slicing, null_readers=True)
    want, dup_needs = streamed(dup, None, slicing)
    for need, dup_need in zip(needs, dup_needs):
        for c in range(NCH):
            if MAP[c] != c:
                assert need[c] == (need[MAP[c]][0], 0), "reader %d: count 0, first its root's" % c
            else:
                assert need[c] == dup_need[c], "root %d: what it brings without a map" % c
    assert sum(n[2][1] for n in needs) == 17003 and sum(n[0][1] for n in needs) == 20000, "every source frame of a root once"
    same(got, want, "streamed %s against the duplicated streamed run" % (slicing,))
    same(got, one_call(mapped, MAP), "streamed %s against the one-call mapped run" % (slicing,))


# ---- a wide fan ----------------------------------------------------------------------------------------------------------------------
def test_wide_fan_of_70_rows():
    """70 channels with empty chains read one 44.1 kHz source of one block and a few frames: the fan crosses any grouping of 64"""
    n = 70
    src = (file_bytes("lpcm16", 7600, 1, 5, 44100), "lpcm16", 44100)
    got = one_call([src] + [None] * (n - 1), [0] * n, 2, count=n, chains=False)
    want = one_call([src] * n, None, 2, count=n, chains=False)
    same(got, want, "70 readers of one root")
    assert len(got[0][0]) == 2 * BLOCK * 3 and any(got[0][0][BLOCK * 3:]), "8272 samples: the second block holds some"
    assert all(o == got[0][0] for o in got[0][:n]), "all 70 outputs are equal to each other"
    assert got[3][1] * n == want[3][1] and got[3][1] == 8272, "the Lanczos sum once per output sample, not once per row"
    assert got[3][0] * n == want[3][0] == n * 7600 * 2


# ---- a reader whose root is empty ----------------------------------------------------------------------------------------------------
def test_reader_of_an_empty_root_is_silent():
    a, b = source_a(), source_b()
    source = [0, 0, 2, 2, 4, 4]
    got = one_call([a, None, None, None, b, None], source)
    want = one_call([a, a, None, None, b, b], None)
    same(got, want, "an empty root")
    assert not any(got[0][3]) and any(got[0][4]), "the reader of the empty root is silent; the job's length comes from the other roots"
    # the reader's own entry is never looked at, whatever it holds
    junk = (file_bytes("lpcm32", 5000, 1, 9, 96000), "lpcm32", 96000)
    ctx = configured()
    ctx.batch_set_sources(source)
    outs = ctx.batch_run([a, junk, None, junk, b, junk], RATE, OUT, **KW)
    ctx.close()
    assert [o.tobytes() for o in outs] == want[0], "a reader's entry is ignored: the roots' samples"


# ---- shards --------------------------------------------------------------------------------------------------------------------------
SPLIT = [(0, 3), (3, 3)]
SHARD_MAPS = [[0, 0, 2], [0, 1, 1]]


def shard_inputs():
    a, b = source_a(), source_b()
    return [[a, None, b], [a, b, None]], [[a, a, b], [a, b, b]]


def sharded(inputs, maps, slicing=None):
    """two contexts of three channels; run_shard + finish_master (slicing None) or the streamed shard form"""
    ctxs = [configured(f, n, 1) for f, n in SPLIT]
    for g, ctx in enumerate(ctxs):
        if maps is not None:
            ctx.batch_set_sources(maps[g])
    job = 3 * BLOCK
    if slicing is None:
        res = [ctx.batch_run_shard(inputs[g], RATE, OUT, job_samples=job, metronome=(g == 0), **KW_SHARD) for g, ctx in enumerate(ctxs)]
        reps = [ctx.batch_report().tobytes() for ctx in ctxs]
        master = ctxs[0].batch_finish_master(OUT, [r[1] for r in res], [r[2] for r in res], aux=res[0][4], sample_rate=RATE, run_meters=True)
        files = [o.tobytes() for r in res for o in r[0]] + [m.tobytes() for m in master] + [res[0][3].tobytes()]
        partial = [(r[1].tobytes(), r[2].tobytes()) for r in res] + [res[0][4].tobytes()]
    else:
        gens = []
        for g, ctx in enumerate(ctxs):
            it = iter(slicing)
            gens.append(ctx.batch_stream_shard(inputs[g], RATE, OUT, lambda left, it=it: next(it), job_samples=job, metronome=(g == 0), **KW_SHARD))
        pieces, reps = [], [b"", b""]
        for k in slicing:
            parts = [next(gen) for gen in gens]
            reps = [r + ctx.batch_report().tobytes() for r, ctx in zip(reps, ctxs)]
            master = ctxs[0].batch_finish_master_slice(OUT, [p[1] for p in parts], [p[2] for p in parts], aux=parts[0][4], sample_rate=RATE, run_meters=True)
            pieces.append((parts, master))
        for gen in gens:
            assert next(gen, None) is None
        files = [b"".join(p[g][0][c].tobytes() for p, _ in pieces) for g in range(2) for c in range(3)]
        files += [b"".join(m[side].tobytes() for _, m in pieces) for side in range(2)] + [b"".join(p[0][3].tobytes() for p, _ in pieces)]
        partial = [tuple(b"".join(p[g][s].tobytes() for p, _ in pieces) for s in (1, 2)) for g in range(2)] + [b"".join(p[0][4].tobytes() for p, _ in pieces)]
    left = [after(ctx, 9) for ctx in ctxs]
    for ctx in ctxs:
        ctx.close()
    return files, partial, reps, left


def test_shards_with_the_map_inside_each_shard():
    mapped, dup = shard_inputs()
    want = sharded(dup, None)
    got = sharded(mapped, SHARD_MAPS)
    assert got[0] == want[0], "the N + 3 files"
    assert got[1] == want[1], "the shards' partial master mixes and the metronome's float64 track"
    assert got[2] == want[2], "the shards' reports"
    assert got[3] == want[3], "meters, tuner and state of both shards"
    streamed_got = sharded(mapped, SHARD_MAPS, (1, 2))
    assert streamed_got[0] == want[0] and streamed_got[1] == want[1], "the streamed shard form in two slices"
    assert streamed_got[3] == want[3]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_a_malformed_map_is_refused_and_the_old_one_stays():
    pkg = package()
    mapped, _ = core_inputs()
    ctx = configured()
    ctx.batch_set_sources(MAP)
    for bad, names in (([0, 0, 2, 0, 6, 5], "channel 4"), ([0, 0, 2, 0, -1, 5], "channel 4"), ([0, 0, 1, 0, 2, 5], "channel 2"),
                       ([0, 0, 2, 0, 2], "5 entries"), ([0, 0, 2, 0, 2, 5, 6], "7 entries")):
        with pytest.raises(pkg.GdgError) as e:
            ctx.batch_set_sources(bad)
        assert e.value.code == pkg.GDG_ERR_INVALID and names in str(e.value), (bad, str(e.value))
    outs = ctx.batch_run(mapped, RATE, OUT, **KW)
    assert [o.tobytes() for o in outs] == duplicated(1)[0], "the map set before the refusals is still in force"
    ctx.close()


def test_the_map_cannot_change_under_an_open_job_and_clearing_restores_independent_inputs():
    pkg = package()
    mapped, dup = core_inputs()
    ctx = configured()
    ctx.batch_set_sources(MAP)
    metas, datas, widths = ctx._stream_split(mapped)
    ctx.batch_stream_open(metas, RATE, OUT, **KW)
    for change in (None, list(range(NCH)), MAP):
        with pytest.raises(pkg.GdgError) as e:
            ctx.batch_set_sources(change)
        assert e.value.code == pkg.GDG_ERR_INVALID and "open" in str(e.value)
    ctx.batch_stream_close()
    ctx.close()
    # cleared: every channel reads its own entry again -- a job with different files per channel, against a context that never had a map
    files = [(file_bytes("lpcm16", 9000 + 1000 * c, 1, 20 + c, RATE), "lpcm16", RATE) for c in range(NCH)]
    ctx = configured()
    ctx.batch_set_sources(MAP)
    ctx.batch_run(mapped, RATE, OUT, **KW)
    ctx.batch_set_sources(None)
    got = [o.tobytes() for o in ctx.batch_run(files, RATE, OUT, **KW)]
    ctx.close()
    never = configured()
    never.batch_run(dup, RATE, OUT, **KW)                           # the units carry the first job's state into the second, as above
    want = [o.tobytes() for o in never.batch_run(files, RATE, OUT, **KW)]
    never.close()
    assert got == want and len(set(got[:NCH])) == NCH
    # a map cleared, or an identity map, before the first job: the buffers of a context that never heard of the call (they only grow,
    # so the comparison is between fresh contexts running the same one job)
    sizes = []
    for source in ("never", None, list(range(NCH))):
        fresh = configured()
        if source != "never":
            fresh.batch_set_sources(MAP)
            fresh.batch_set_sources(source)
        outs = [o.tobytes() for o in fresh.batch_run(files, RATE, OUT, **KW)]
        sizes.append((fresh.get_option("stat_batch_device_kib"), outs))
        fresh.close()
    assert sizes[1] == sizes[0] and sizes[2] == sizes[0]


def test_checkpoints_are_refused_with_a_reader_and_work_with_an_identity_map():
    pkg = package()
    mapped, dup = core_inputs()
    ctx = configured()
    ctx.batch_set_sources(MAP)
    metas, datas, widths = ctx._stream_split(mapped)
    ctx.batch_stream_open(metas, RATE, OUT, **KW)
    import ctypes as C
    size = C.c_size_t(0)
    assert pkg.lib().gdg_batch_stream_checkpoint_size(ctx._h, C.byref(size)) == pkg.GDG_ERR_UNSUPPORTED
    assert "shared sources" in pkg.lib().gdg_last_error(ctx._h).decode()
    buf = C.create_string_buffer(64)
    assert pkg.lib().gdg_batch_stream_checkpoint(ctx._h, buf, 64, None) == pkg.GDG_ERR_UNSUPPORTED
    assert "shared sources" in pkg.lib().gdg_last_error(ctx._h).decode()
    ctx.batch_stream_close()
    for resume in (lambda: ctx.batch_stream_resume(metas, RATE, OUT, b"\0" * 64, **KW),
                   lambda: ctx.batch_stream_resume_shard(metas, RATE, OUT, b"\0" * 64, **KW_SHARD)):
        with pytest.raises(pkg.GdgError) as e:
            resume()
        assert e.value.code == pkg.GDG_ERR_UNSUPPORTED and "shared sources" in str(e.value)
    ctx.close()
    # an identity map is no map: checkpoint after the first block, resume in a fresh context, the uninterrupted bytes
    want = duplicated(1)
    src = configured()
    src.batch_set_sources(list(range(NCH)))
    metas, datas, widths = src._stream_split(dup)
    src.batch_stream_open(metas, RATE, OUT, **KW)
    feed = lambda c, k: [None if d is None or not n else d[f * w:(f + n) * w] for d, w, (f, n) in zip(datas, widths, c.batch_stream_need(k))]
    head = src.batch_stream_step(1, feed(src, 1))
    blob = src.batch_stream_checkpoint()
    src.close()
    dst = configured()
    dst.batch_set_sources(list(range(NCH)))
    assert dst.batch_stream_resume(metas, RATE, OUT, blob, **KW) == BLOCK
    tail = dst.batch_stream_step(2, feed(dst, 2))
    dst.batch_stream_close()
    left = after(dst, 2 * NCH + 3)
    dst.close()
    assert [h.tobytes() + t.tobytes() for h, t in zip(head, tail)] == want[0]
    assert left == want[1]
