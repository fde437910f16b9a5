"""Channel state saved and loaded (gdg_state_*, api_state.cpp, state.hip): a save changes nothing, a load puts a context -- the same one,
or another with another channel count, window or group setting -- exactly where the source was, and a load that does not fit changes
nothing.  The bench chain of test_gpu_fir_ahead.py at 192 kHz, 8192-sample frames, unless a test says otherwise; GDG_PLAN_TRACE=2 shows
which launch shapes the calls around the save and the load took."""
import numpy as np
import pytest

import __graft_entry__ as entry
from helpers import TOL_RMS, launches, rms, synth_ir, synth_signal

pytestmark = pytest.mark.gpu
FRAMES = 8192
SR = 192000
TAPS = 65536                                      # K = 8 at 8192-sample frames
HEAD = [("compressor", [1, 30, -20]), ("overdrive", [0, 20, 100, 0, 1, 0]), ("tone_stack", None), ("chorus", None)]
BENCH = HEAD + [("power_amp", "a"), ("power_amp", "b"), ("cabinet", None), ("reverb", [50])]
IRS = {"a": lambda c: synth_ir(TAPS, seed=5), "b": lambda c: synth_ir(TAPS, seed=6)}


@pytest.fixture(scope="module")
def pkg():
    return entry.load_package()


@pytest.fixture(scope="module")
def oracle():
    o = entry.load_oracle()
    o.build()
    return o


def make(pkg, nch, chain=BENCH, irs=IRS, groups=0, window=0, options=None, frames=FRAMES):
    ctx = pkg.Context(nch, frames)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    if groups:
        ctx.set_overlap(groups)
    if window:
        ctx.set_window(window)
    for c in range(nch):
        for name, p in chain:
            if isinstance(p, str):
                ctx.append_unit(c, name, fir=irs[p](c))
            else:
                ctx.append_unit(c, name, params=p)
    return ctx


def signal(nch, blocks, c0=0, frames=FRAMES, sr=SR):
    return np.stack([synth_signal(c + c0, frames * blocks, sr) for c in range(nch)])


class Stream:
    """Per-frame device-resident calls of a context, one block of `x` after another, back to back: every input is uploaded before the
    first call and every output downloaded after the last (a copy between the calls would drop the sums made ahead of the next frame)."""

    def __init__(self, ctx, nch, frames=FRAMES, sr=SR):
        self.ctx, self.nch, self.frames, self.sr = ctx, nch, frames, sr

    def run(self, x, b0, n, each=None):
        f = self.frames
        d_in = [self.ctx.alloc(self.nch, f) for _ in range(n)]
        d_out = [self.ctx.alloc(self.nch, f) for _ in range(n)]
        for i, d in enumerate(d_in):
            d.upload(np.ascontiguousarray(x[:, (b0 + i) * f:(b0 + i + 1) * f]))
        for i in range(n):
            self.ctx.process_device(d_in[i], d_out[i], f, self.sr)
            if each is not None:
                each(self.ctx)
        out = np.concatenate([d.download() for d in d_out], axis=1)
        for d in d_in + d_out:
            d.free()
        return out

    def free(self):
        pass


def counters(ctx):
    return ctx.get_option("stat_fir_ahead_sums_used"), ctx.get_option("stat_premac_launches_used")


# ---- 1. rollback -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,groups,shape", [(3, 0, "SEGT"), (64, 0, "PREMAC"), (160, 0, "SPLIT"), (512, 2, "AHEAD")])
def test_rollback_gives_the_same_bits(pkg, capfd, monkeypatch, nch, groups, shape):
    """5 blocks, save, 6 more (A); load, the same 6 again (B).  The trace of A (between the save and the load) and of B must show the shape."""
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    ctx = make(pkg, nch, groups=groups)
    x = signal(nch, 11)
    s = Stream(ctx, nch)
    s.run(x, 0, 5)
    blob = ctx.save_state()
    capfd.readouterr()
    used0 = counters(ctx)
    a = s.run(x, 5, 6)
    lines_a = launches(capfd.readouterr().err)
    ctx.synchronize()
    used_a = counters(ctx)
    ctx.load_state(blob)
    ctx.synchronize()
    used1 = counters(ctx)
    b_first = s.run(x, 5, 1)
    ctx.synchronize()
    used2 = counters(ctx)
    b = np.concatenate([b_first, s.run(x, 6, 5)], axis=1)
    lines_b = launches(capfd.readouterr().err)
    ctx.close()
    # the trace names the premac launches PREMAC and the pass of the sums made ahead AHEAD
    for lines in (lines_a, lines_b):
        assert shape in {r["shape"] for r in lines}, {r["shape"] for r in lines}
        if nch == 64:       # the reverb's wet path made ahead by the first segment launch (seg.hip REVERB_AHEAD)
            assert any(r["shape"] in ("SEGT", "GENERAL_AHEAD") and r["ahead"] > 0 for r in lines), lines
    if nch == 512:
        assert used_a[0] > used0[0]                 # A continued sums made ahead ...
    if nch == 64:
        assert used_a[1] > used0[1]                 # ... or premac sums
        # the first call after the load continued no premac sum made before it (the load dropped it)
        assert used2[1] == used1[1], (used1, used2)
    # the sums made ahead of a new epoch start in the first call itself: its bits show that nothing stale was read
    assert np.array_equal(a, b)


# ---- 2. a save is invisible ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch,groups", [(64, 0), (512, 2)])
def test_a_save_after_every_block_changes_nothing(pkg, nch, groups):
    x = signal(nch, 8)
    res = []
    for save in (False, True):
        ctx = make(pkg, nch, groups=groups)
        s = Stream(ctx, nch)
        blobs = []
        out = s.run(x, 0, 8, each=(lambda c: blobs.append(len(c.save_state()))) if save else None)
        ctx.synchronize()
        res.append((out, counters(ctx)))
        s.free()
        ctx.close()
    assert np.array_equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1], (res[0][1], res[1][1])
    assert res[0][1][0] > 0 or res[0][1][1] > 0


# ---- 3. migration ----------------------------------------------------------------------------------------------------------------
def _oracle_chain(oracle, c):
    ch = oracle.Chain()
    for name, p in BENCH:
        if isinstance(p, str):
            ch.append_unit(name, fir=IRS[p](c))
        else:
            ch.append_unit(name, params=p)
    return ch


@pytest.mark.parametrize("variant", ["window", "window_reverse", "groups", "channels"])
def test_migration_continues_the_source_channels(pkg, oracle, variant):
    """A (8 channels) saves channels [5, 2]; B loads them into its channels [1, 0].  "window": B runs a window of 16 frames after the
    load; "window_reverse": A ran one window of 16 frames before the save, B continues per frame; "groups": B with two channel groups;
    "channels": B with 5 channels instead of 3."""
    src, dst = [5, 2], [1, 0]
    k = 16 if variant == "window_reverse" else 3
    m = 16 if variant == "window" else 3
    x = signal(8, k + m)
    a = make(pkg, 8, window=16 if variant == "window_reverse" else 0)
    if variant == "window_reverse":
        d, o = a.alloc(8, 16 * FRAMES), a.alloc(8, 16 * FRAMES)
        d.upload(np.ascontiguousarray(x[:, :16 * FRAMES]))
        a.process_window_device(d.ptr, o.ptr, 16 * FRAMES, 16, SR)
        a.synchronize()
        head = o.download()
        d.free()
        o.free()
    sa = Stream(a, 8)
    if variant != "window_reverse":
        head = sa.run(x, 0, k)
    blob = a.save_state(src)
    want = sa.run(x, k, m)                          # A's continuation, per frame
    sa.free()
    a.close()
    nb = 5 if variant == "channels" else 3
    b = make(pkg, nb, window=16 if variant == "window" else 0, groups=2 if variant == "groups" else 0)
    b.load_state(blob, dst)
    xb = np.zeros((nb, x.shape[1]))
    for i, c in zip(dst, src):
        xb[i] = x[c]
    if variant == "window":
        d, o = b.alloc(nb, 16 * FRAMES), b.alloc(nb, 16 * FRAMES)
        d.upload(np.ascontiguousarray(xb[:, k * FRAMES:]))
        b.process_window_device(d.ptr, o.ptr, 16 * FRAMES, 16, SR)
        b.synchronize()
        got_all = o.download()
        d.free()
        o.free()
    else:
        sb = Stream(b, nb)
        got_all = sb.run(xb, k, m)
        sb.free()
    b.close()
    for i, c in zip(dst, src):
        got, ref = got_all[i], want[c]
        assert np.array_equal(got, ref), (variant, c, rms(got - ref))
        ch = _oracle_chain(oracle, c)               # the oracle over the whole stream from zero
        whole = np.concatenate([ch.process(x[c, bb * FRAMES:(bb + 1) * FRAMES], SR) for bb in range(k + m)])
        assert rms(head[c] - whole[:k * FRAMES]) <= TOL_RMS
        assert rms(got - whole[k * FRAMES:]) <= TOL_RMS, rms(got - whole[k * FRAMES:])


# ---- 4. every unit type ----------------------------------------------------------------------------------------------------------
SR_UNITS = 48000
UNIT_CASES = [
    ("signal_generator", [100, 0, 4, 440, 100, 0]), ("noise_gate", None), ("bandpass", [2, 300, 3000]), ("auto_wah", None), ("auto_yoy", None),
    ("compressor", None), ("octaver", None), ("excess", [0, 0, 1]), ("excess", [0, 0, 2]), ("fuzz", [1, 50, 0, 0, 100, 0, 1]),
    ("fuzz", [1, 50, 0, 0, 100, 0, 2]), ("overdrive", [0, 20, 100, 0, 1, 1]), ("overdrive", [0, 20, 100, 0, 1, 2]),
    ("distortion", [0, 0, 0, 1]), ("distortion", [0, 0, 0, 2]), ("tone_stack", None), ("chorus", None), ("flanger", None), ("phaser", None),
    ("tremolo", None), ("ring_modulator", None), ("delay", None), ("reverb", None), ("power_amp", "fir"), ("cabinet", None),
]


@pytest.mark.parametrize("name,params", UNIT_CASES, ids=["%s-%d" % (c[0], i) for i, c in enumerate(UNIT_CASES)])
def test_every_unit_type_continues_bit_for_bit(pkg, name, params):
    nch, pre, post = 2, 5, 3
    chain = [(name, "a" if params == "fir" else params)]
    irs = {"a": lambda c: synth_ir(20000, seed=30 + c)}
    x = 0.8 * signal(nch, pre + post, c0=11, sr=SR_UNITS)
    x[:, pre * FRAMES:] *= 0.01                     # a quiet continuation: followers, gates and filters still carry the loud part
    a = make(pkg, nch, chain, irs)
    sa = Stream(a, nch, sr=SR_UNITS)
    sa.run(x, 0, pre)
    blob = a.save_state()
    want = sa.run(x, pre, post)
    b = make(pkg, nch, chain, irs)
    b.load_state(blob)
    sb = Stream(b, nch, sr=SR_UNITS)
    got = sb.run(x, pre, post)
    # a fresh context without the load differs: the state mattered
    c = make(pkg, nch, chain, irs)
    sc = Stream(c, nch, sr=SR_UNITS)
    cold = sc.run(x, pre, post)
    for s, ctx in ((sa, a), (sb, b), (sc, c)):
        s.free()
        ctx.close()
    assert np.array_equal(got, want), name
    assert not np.array_equal(cold, want), name     # without the load the continuation differs: the state mattered


# ---- 5. another frame size after the load ----------------------------------------------------------------------------------------
def test_frame_size_after_a_load(pkg, oracle):
    nch = 2
    x = signal(nch, 6)
    a = make(pkg, nch)
    sa = Stream(a, nch)
    sa.run(x, 0, 3)
    blob = a.save_state()
    b = make(pkg, nch)
    b.load_state(blob)
    half = 4096
    tail = x[:, 3 * FRAMES:]
    sa2, sb2 = Stream(a, nch, frames=half), Stream(b, nch, frames=half)
    want = sa2.run(tail, 0, 6)
    got = sb2.run(tail, 0, 6)
    for s, ctx in ((sa, None), (sa2, a), (sb2, b)):
        s.free()
        if ctx is not None:
            ctx.close()
    assert np.array_equal(got, want)
    for c in range(nch):
        ch = _oracle_chain(oracle, c)
        head = [ch.process(x[c, bb * FRAMES:(bb + 1) * FRAMES], SR) for bb in range(3)]
        ref = np.concatenate([ch.process(tail[c, bb * half:(bb + 1) * half], SR) for bb in range(6)])
        assert rms(got[c] - ref) <= TOL_RMS, rms(got[c] - ref)
        del head


# ---- 6. spatializer --------------------------------------------------------------------------------------------------------------
def test_spatializer_history_moves_with_the_channels(pkg):
    """A (4 channels) spatializes 3 blocks, saves channels [3, 1]; B (3 channels) loads them into [0, 2].  The channels that do not move
    mix at level 0 (their terms are exact zeros), so A's and B's mixes of the next blocks are the same sums: bit-equal."""
    src, dst = [3, 1], [0, 2]
    x = signal(4, 5)
    a, b = make(pkg, 4), make(pkg, 3)
    pos = {c: (30.0 * c - 45.0, 1.0 + 0.5 * c, 0.8) for c in range(4)}
    for c in range(4):
        a.spatializer_set_position(c, *(pos[c] if c in src else (0.0, 1.0, 0.0)))
    b.spatializer_set_position(1, 0.0, 1.0, 0.0)
    for i, c in zip(dst, src):
        b.spatializer_set_position(i, *pos[c])
    sa = Stream(a, 4)
    for bb in range(3):
        a.spatialize(sa.run(x, bb, 1))
    b.load_state(a.save_state(src), dst)
    sb = Stream(b, 3)
    xb = np.zeros((3, x.shape[1]))
    for i, c in zip(dst, src):
        xb[i] = x[c]
    for bb in range(3, 5):
        ya, yb = sa.run(x, bb, 1), sb.run(xb, bb, 1)
        for i, c in zip(dst, src):
            assert np.array_equal(ya[c], yb[i])
        yb[1] = 0.0
        la, lb = a.spatialize(ya), b.spatialize(yb)
        assert all(np.array_equal(p, q) for p, q in zip(la, lb)), bb
    a.close()
    b.close()


# ---- 7. rejections ---------------------------------------------------------------------------------------------------------------
SMALL = [("compressor", [1, 30, -20]), ("delay", [200, -5, -5]), ("power_amp", "a"), ("cabinet", None)]
SMALL_IRS = {"a": lambda c: synth_ir(3 * FRAMES, seed=9)}


def _corrupt(blob, at, value):
    b = bytearray(blob)
    b[at:at + len(value)] = value
    return bytes(b)


@pytest.mark.parametrize("case", ["order", "filter_length", "delay_time", "magic", "version", "truncated", "wrong_n", "capacity"])
def test_a_rejected_load_changes_nothing(pkg, case):
    nch = 2
    x = signal(nch, 5, c0=4)
    src = make(pkg, nch, SMALL, SMALL_IRS)
    ss = Stream(src, nch)
    ss.run(x, 0, 2)
    blob = src.save_state()
    chain, irs, channels = SMALL, SMALL_IRS, None
    if case == "order":
        chain = [SMALL[1], SMALL[0]] + SMALL[2:]
    elif case == "filter_length":
        irs = {"a": lambda c: synth_ir(5 * FRAMES, seed=9)}
    elif case == "delay_time":
        chain = [SMALL[0], ("delay", [300, -5, -5])] + SMALL[2:]
    elif case == "magic":
        blob = _corrupt(blob, 0, b"XDGSTATE")
    elif case == "version":
        blob = _corrupt(blob, 8, (99).to_bytes(4, "little"))
    elif case == "truncated":
        blob = blob[:len(blob) - 100]
    elif case == "wrong_n":
        channels = [0]
    target, twin = make(pkg, nch, chain, irs), make(pkg, nch, chain, irs)
    st, sw = Stream(target, nch), Stream(twin, nch)
    st.run(x, 0, 1)
    sw.run(x, 0, 1)
    if case == "capacity":
        import ctypes as C
        lib = pkg.lib()
        need = src.state_size()
        buf = C.create_string_buffer(need)
        written = C.c_size_t(0)
        rc = lib.gdg_state_save(src._h, None, 0, buf, need - 16, C.byref(written))
        assert rc == pkg.GDG_ERR_INVALID and written.value == need
        assert "capacity" in lib.gdg_last_error(src._h).decode()
    else:
        with pytest.raises(pkg.GdgError) as e:
            target.load_state(blob, channels)
        assert e.value.code == pkg.GDG_ERR_INVALID
        msg = str(e.value)
        if case in ("order", "filter_length", "delay_time"):
            assert "channel 0" in msg and "slot" in msg, msg
            key = {"order": "unit type", "filter_length": "K", "delay_time": "hist_"}[case]
            assert key in msg, msg
    got, want = st.run(x, 1, 3), sw.run(x, 1, 3)
    for s, ctx in ((ss, src), (st, target), (sw, twin)):
        s.free()
        ctx.close()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("frames,rate", [(4096, SR), (FRAMES, 96000)])
def test_a_rejected_load_leaves_a_target_at_another_frame_size_or_rate_alone(pkg, frames, rate):
    """The blob is laid out at 8192 frames / 192 kHz, the target runs at another frame size or rate, and its LAST channel has another
    delay time: the load is rejected, and channel 0 -- which a load lays out at the blob's frame size and rate -- must continue exactly
    like a twin's."""
    nch = 2
    x = signal(nch, 5, c0=4)
    src = make(pkg, nch, SMALL, SMALL_IRS)
    Stream(src, nch).run(x, 0, 2)
    blob = src.save_state()
    src.close()

    def target():
        ctx = pkg.Context(nch, FRAMES)
        for c in range(nch):
            for name, p in SMALL:
                if name == "delay" and c == nch - 1:
                    p = [300, -5, -5]
                if isinstance(p, str):
                    ctx.append_unit(c, name, fir=SMALL_IRS[p](c))
                else:
                    ctx.append_unit(c, name, params=p)
        return ctx
    t, w = target(), target()
    xt = signal(nch, 6, c0=9, frames=frames, sr=rate)
    st, sw = Stream(t, nch, frames=frames, sr=rate), Stream(w, nch, frames=frames, sr=rate)
    st.run(xt, 0, 3)
    sw.run(xt, 0, 3)
    with pytest.raises(pkg.GdgError) as e:
        t.load_state(blob)
    assert "channel 1" in str(e.value) and "hist_" in str(e.value), str(e.value)
    got, want = st.run(xt, 3, 3), sw.run(xt, 3, 3)
    t.close()
    w.close()
    assert np.array_equal(got, want)


# ---- 8. host and device blobs ----------------------------------------------------------------------------------------------------
def test_host_and_device_blobs_are_the_same_bytes(pkg):
    nch = 3
    x = signal(nch, 5)
    a = make(pkg, nch)
    sa = Stream(a, nch)
    sa.run(x, 0, 3)
    host = a.save_state([2, 0])
    size = a.state_size([2, 0])
    assert size == len(host) and size % 16 == 0
    d = a.alloc(1, (size + 7) // 8)
    assert a.save_state_device(d, [2, 0]) == size
    assert d.download().tobytes()[:size] == host
    want = sa.run(x, 3, 2)
    outs = []
    for kind in ("host", "device"):
        b = make(pkg, nch)
        if kind == "host":
            b.load_state(host, [2, 0])
        else:
            db = b.alloc(1, (size + 7) // 8)
            arr = np.frombuffer(host + b"\0" * (db.cols * 8 - size), dtype=np.float64).reshape(1, -1)
            db.upload(arr)
            b.load_state_device(db, size, [2, 0])
            db.free()
        sb = Stream(b, nch)
        outs.append(sb.run(x, 3, 2))
        sb.free()
        b.close()
    d.free()
    sa.free()
    a.close()
    for o in outs:
        assert np.array_equal(o[2], want[2]) and np.array_equal(o[0], want[0])


# ---- 9. edge cases ---------------------------------------------------------------------------------------------------------------
def test_a_unit_that_never_ran_loads_as_a_reset(pkg):
    nch = 2
    x = signal(nch, 4)
    fresh = make(pkg, nch)
    blob = fresh.save_state()                       # never processed: every slot fresh
    used = make(pkg, nch)
    su = Stream(used, nch)
    su.run(x, 0, 2)
    used.load_state(blob)
    ref = make(pkg, nch)
    sr_ = Stream(ref, nch)
    got, want = su.run(x, 2, 2), sr_.run(x, 2, 2)
    for s, ctx in ((su, used), (sr_, ref)):
        s.free()
        ctx.close()
    fresh.close()
    assert np.array_equal(got, want)


def test_set_fir_after_a_load_still_resets(pkg):
    nch = 1
    chain = [("power_amp", "a")]
    irs = {"a": lambda c: synth_ir(3 * FRAMES, seed=12)}
    x = signal(nch, 4)
    a = make(pkg, nch, chain, irs)
    sa = Stream(a, nch)
    sa.run(x, 0, 2)
    blob = a.save_state()
    b = make(pkg, nch, chain, irs)
    b.load_state(blob)
    b.unit_set_fir(0, synth_ir(3 * FRAMES, seed=13))
    c = make(pkg, nch, chain, {"a": lambda c: synth_ir(3 * FRAMES, seed=13)})
    sb, sc = Stream(b, nch), Stream(c, nch)
    got, want = sb.run(x, 2, 2), sc.run(x, 2, 2)
    for s, ctx in ((sa, a), (sb, b), (sc, c)):
        s.free()
        ctx.close()
    assert np.array_equal(got, want)


# ---- 10. two devices -------------------------------------------------------------------------------------------------------------
def test_a_blob_moves_between_devices(pkg):
    if pkg.device_count() < 2:
        pytest.skip("one device visible")
    nch = 2
    x = signal(nch, 5)
    a = pkg.Context(nch, FRAMES, device=0)
    b = pkg.Context(nch, FRAMES, device=1)
    for ctx in (a, b):
        for c in range(nch):
            for name, p in SMALL:
                if isinstance(p, str):
                    ctx.append_unit(c, name, fir=SMALL_IRS[p](c))
                else:
                    ctx.append_unit(c, name, params=p)
    sa = Stream(a, nch)
    sa.run(x, 0, 3)
    b.load_state(a.save_state())
    sb = Stream(b, nch)
    got, want = sb.run(x, 3, 2), sa.run(x, 3, 2)
    for s, ctx in ((sa, a), (sb, b)):
        s.free()
        ctx.close()
    assert np.array_equal(got, want)


# ---- 11. the C++ twin: an engine over 3 contexts saves, one over 2 loads ---------------------------------------------------------
def test_engine_state_moves_to_another_shard_count(pkg, oracle):
    from go_dsp_guitar_amd import host
    host.build()
    sr, frames, nch, k, m = 48000, 1024, 7, 3, 3
    taps = {"Cab": synth_ir(2000, seed=3), "Room": synth_ir(5000, seed=4)}
    irs = host.ImpulseResponses()
    irs.add("Cab", sr, -20, taps["Cab"])
    irs.add("Room", sr, -10, taps["Room"])
    spec = [(5, {"gain_limit": 30, "target_level": -20}), (9, {"gain": 20}), (11, {}), (12, {}), (19, None), (20, {}), (18, {"mix": 50})]

    def engine(devices):
        eng = host.Engine(nch, frames, devices=devices)
        for _ in range(nch):
            ch = eng.create_chain(irs)
            for t, numeric in spec:
                i = ch.AppendUnit(t)
                if t == 19:
                    ch.SetDiscreteValue(i, "filter_1", "Cab")
                    ch.SetNumericValue(i, "level_1", -3)
                    ch.SetDiscreteValue(i, "filter_2", "Room")
                else:
                    for key, v in numeric.items():
                        ch.SetNumericValue(i, key, v)
                ch.SetBypass(i, False)
        return eng
    x = np.stack([synth_signal(c, frames * (k + m), sr) for c in range(nch)])
    blk = [np.ascontiguousarray(x[:, b * frames:(b + 1) * frames]) for b in range(k + m)]
    a = engine([0, 0, 0])
    assert a.shards() == 3
    head = [a.process_all(blk[b], sr) for b in range(k)]
    blob = a.save_state()
    want = np.concatenate([a.process_all(blk[b], sr) for b in range(k, k + m)], axis=1)
    b2 = engine([0, 0])
    assert b2.shards() == 2
    b2.load_state(blob, sr)
    got = np.concatenate([b2.process_all(blk[b], sr) for b in range(k, k + m)], axis=1)
    assert a.last_error() == "" and b2.last_error() == ""
    a.close()
    b2.close()
    assert np.array_equal(got, want)
    # the oracle's pipeline over the whole stream
    fa = oracle.Filter(taps["Cab"], sr, 10.0 ** (0.05 * -20)).normalize().multiply(10.0 ** (0.05 * -3))
    fb = oracle.Filter(taps["Room"], sr, 10.0 ** (0.05 * -10)).normalize().multiply(1.0)
    composite = oracle.Filter([], sr).add(fa).add(fb).coefficients()
    for c in (0, 3, 6):
        ref = oracle.Chain()
        ref.append_unit("compressor", params=[1, 30, -20])
        ref.append_unit("overdrive", params=[0, 20, 100, 0, 1, 0])
        ref.append_unit("tone_stack")
        ref.append_unit("chorus")
        ref.append_unit("power_amp", fir=composite)
        ref.append_unit("cabinet")
        ref.append_unit("reverb", params=[50])
        whole = np.concatenate([ref.process(blk[b][c], sr) for b in range(k + m)])
        assert rms(np.concatenate([h[c] for h in head]) - whole[:k * frames]) <= TOL_RMS
        assert rms(got[c] - whole[k * frames:]) <= TOL_RMS, (c, rms(got[c] - whole[k * frames:]))
