"""Per-frame calls of many channels: a pass at the start of call t0 sums, for a 1/T share of the channels, the terms k >= j + 1 of frames
t0 + j (j < T) -- the ones that only read frames already in the delay line -- and the inverse kernel of frame t0 + j adds the terms k = j .. 0
(fir_ahead_kernel, fir_inv_kernel FUSED 5 / 6, api_process.cpp).  Every multiply-accumulate kernel sums k descending, so the sums must have
the bits of the whole sum; anything but a per-frame call of the same plan must make the next calls sum everything again."""
import numpy as np
import pytest

import __graft_entry__ as entry
from helpers import ChainPair, TOL_RMS, launches, rms, synth_ir, synth_signal

pytestmark = pytest.mark.gpu
FRAMES = 8192
SR = 192000
T = 4
TAPS = 65536                                      # K = 8 at 8192-sample frames
HEAD = [("compressor", [1, 30, -20]), ("overdrive", [0, 20, 100, 0, 1, 0]), ("tone_stack", None), ("chorus", None)]
BENCH = HEAD + [("power_amp", "a"), ("power_amp", "b"), ("cabinet", None), ("reverb", [50])]


@pytest.fixture(scope="module")
def pkg():
    return entry.load_package()


@pytest.fixture(scope="module")
def oracle():
    o = entry.load_oracle()
    o.build()
    return o


def make(pkg, nch, chain, irs, ahead, groups=1, options=None):
    ctx = pkg.Context(nch, FRAMES)
    ctx.set_option("fir_ahead_frames", T if ahead else 0)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    if groups > 1:
        ctx.set_overlap(groups)
    handles = [[] for _ in range(nch)]
    for c in range(nch):
        for name, p in chain:
            if isinstance(p, str):
                handles[c].append(ctx.append_unit(c, name, fir=irs[p](c)))
            else:
                handles[c].append(ctx.append_unit(c, name, params=p))
    return ctx, handles


def resident_calls(ctx, x_blocks, calls, between=None, at=None):
    """`calls` back-to-back per-frame calls on resident inputs (block b % len), each into an output buffer of its own, downloaded at the end;
    `between(ctx)` runs after call `at` (and may return extra outputs of its own)"""
    nch = x_blocks[0].shape[0]
    d_in = [ctx.alloc(nch, FRAMES) for _ in x_blocks]
    for d, x in zip(d_in, x_blocks):
        d.upload(x)
    d_out = [ctx.alloc(nch, FRAMES) for _ in range(calls)]
    extra = []
    for b in range(calls):
        ctx.process_device(d_in[b % len(d_in)], d_out[b], FRAMES, SR)
        if between is not None and b == at:
            extra = between(ctx) or []
    ctx.synchronize()
    used = ctx.get_option("stat_fir_ahead_sums_used")
    outs = [d.download() for d in d_out]
    for d in d_in + d_out:
        d.free()
    return outs, extra, used


def expected_used(n, K, calls, T=T):
    """channel frames that continue sums made ahead, by the stagger: channel i of a launch of n has phase i // ceil(n / T), its sums are
    made at the calls c = phase (mod T) and serve frames j = 0 .. min(T, K - 1) - 1 after that"""
    m = -(-n // T)
    return sum(1 for c in range(calls) for i in range(n) if c >= i // m and (c - i // m) % T < min(T, K - 1))


def blocks(nch, n, c0=0):
    x = np.stack([synth_signal(c + c0, FRAMES * n, SR) for c in range(nch)])
    return [np.ascontiguousarray(x[:, b * FRAMES:(b + 1) * FRAMES]) for b in range(n)]


@pytest.mark.parametrize("nch,groups", [(256, 1), (512, 2)])
def test_bench_chain_gives_the_bits_of_the_whole_sum(pkg, nch, groups):
    """the default thresholds: the bench chain takes the shape at 256 channels per group; 3 T + 1 calls, every one bit-equal"""
    irs = {"a": lambda c: synth_ir(TAPS, seed=5), "b": lambda c: synth_ir(TAPS, seed=6)}
    x = blocks(nch, 4)
    calls = 3 * T + 1
    res = {}
    for ahead in (False, True):
        ctx, _ = make(pkg, nch, BENCH, irs, ahead, groups=groups)
        res[ahead] = resident_calls(ctx, x, calls)
        ctx.close()
    assert res[False][2] == 0
    assert res[True][2] == expected_used(nch // groups, 8, calls) * 2 * groups, res[True][2]          # counted on the device: both amps, every group
    for b in range(calls):
        assert np.array_equal(res[True][0][b], res[False][0][b]), "call %d" % b


def test_the_shape_and_its_pass_in_the_plan_trace(pkg, capfd, monkeypatch):
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    irs = {"a": lambda c: synth_ir(TAPS, seed=5), "b": lambda c: synth_ir(TAPS, seed=6)}
    ctx, _ = make(pkg, 256, BENCH, irs, True)
    capfd.readouterr()
    resident_calls(ctx, blocks(256, 1), 2)
    ctx.close()
    lines = launches(capfd.readouterr().err)
    # the two heads -- fused launches whose `ahead` field is the frames one pass serves -- and the pass's line behind the group's steps
    assert [(r["shape"], r["ahead"]) for r in lines if r["step"] in (1, 2)] == [("FUSED", T), ("FUSED", T), ("AHEAD", 2)] * 2
    assert all(r["n"] == 64 for r in lines if r["shape"] == "AHEAD")


@pytest.mark.parametrize("taps,taken", [(TAPS, True), (5 * FRAMES - 100, True), (3 * FRAMES - 100, False), (FRAMES, False)])
def test_one_amp_by_filter_length(pkg, capfd, monkeypatch, taps, taken):
    """K = 8, K = 5 (the fewest partitions at which the pass moves fewer bytes with T = 4), K = 3 and K = 1 (the shape is not taken)"""
    nch = 12
    irs = {"a": lambda c: synth_ir(taps, seed=40 + c)}
    chain = [("compressor", [1, 30, -20]), ("power_amp", "a"), ("cabinet", None)]
    opts = {"fir_fused": 1, "fir_ahead_min_channels": 1}
    x = blocks(nch, 3, c0=7)
    calls = 3 * T + 1
    res = {}
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    for ahead in (False, True):
        ctx, _ = make(pkg, nch, chain, irs, ahead, options=opts)
        capfd.readouterr()
        res[ahead] = resident_calls(ctx, x, calls)
        lines = launches(capfd.readouterr().err)
        ctx.close()
        assert ("AHEAD" in {r["shape"] for r in lines}) == (ahead and taken)
        assert {r["ahead"] for r in lines if r["shape"] == "FUSED"} == {T if (ahead and taken) else 0}
    K = -(-taps // FRAMES)
    assert res[True][2] == (expected_used(nch, K, calls) if taken else 0), res[True][2]
    for b in range(calls):
        assert np.array_equal(res[True][0][b], res[False][0][b]), "call %d" % b


def test_back_to_back_calls_follow_the_oracle(pkg, oracle):
    nch, calls = 8, 2 * T + 1
    x = blocks(nch, calls, c0=3)
    ctx = pkg.Context(nch, FRAMES)
    ctx.set_option("fir_fused", 1)
    ctx.set_option("fir_ahead_min_channels", 1)
    pairs = []
    for c in range(nch):
        p = ChainPair(ctx, c, oracle)
        p.append("compressor")
        p.append("power_amp", fir=synth_ir(TAPS - 3000, seed=300 + c))
        p.append("power_amp", fir=synth_ir(40000, seed=400 + c))
        p.append("cabinet")
        pairs.append(p)
    outs, _, used = resident_calls(ctx, x, calls)
    ctx.close()
    assert used == expected_used(nch, 8, calls) + expected_used(nch, 5, calls)       # 61536 taps: K = 8; 40000 taps: K = 5
    for c in (0, 3, 7):
        want = np.concatenate([pairs[c].ref.process(x[b][c], SR) for b in range(calls)])
        got = np.concatenate([outs[b][c] for b in range(calls)])
        assert rms(got - want) <= TOL_RMS, (c, rms(got - want))


def _set_fir(ctx, h):
    ctx.unit_set_fir(h[1][2], synth_ir(50000, seed=77))


def _reset(ctx, h):
    ctx.unit_reset(h[2][3])


def _frame_size(ctx, h):
    nch = len(h)
    d_in, d_out = ctx.alloc(nch, 4096), ctx.alloc(nch, 4096)
    d_in.upload(np.stack([synth_signal(c, 4096, SR) for c in range(nch)]))
    ctx.process_device(d_in, d_out, 4096, SR)
    ctx.synchronize()
    return [d_out.download()]


def _window(ctx, h):
    nch = len(h)
    d_in, d_out = ctx.alloc(nch, 2 * FRAMES), ctx.alloc(nch, 2 * FRAMES)
    d_in.upload(np.stack([synth_signal(c + 11, 2 * FRAMES, SR) for c in range(nch)]))
    ctx.set_window(2)
    ctx.process_window_device(d_in.ptr, d_out.ptr, 2 * FRAMES, 2, SR)
    ctx.synchronize()
    return [d_out.download()]


def _chain_edit(ctx, h):
    ctx.chain_set(3, h[3], bypass=[False, False, False, True, False])


def _sharing(ctx, h):
    ctx.share_ir_spectra(False)
    ctx.unit_set_fir(h[0][3], synth_ir(30000, seed=91))


def _plan_rebuild(ctx, h):
    ctx.set_option("seg_tile_max_channels", 0)


@pytest.mark.parametrize("action", [_set_fir, _reset, _frame_size, _window, _chain_edit, _sharing, _plan_rebuild],
                         ids=["set_fir", "reset", "frame_size", "window", "chain_edit", "sharing", "plan_rebuild"])
def test_what_touches_the_context_drops_the_sums(pkg, action):
    """in the middle of a block of T calls: the same outputs as a context that never makes sums ahead, and the count starts over"""
    nch, before, after = 8, 6, 6
    irs = {"a": lambda c: synth_ir(TAPS, seed=500 + c), "b": lambda c: synth_ir(TAPS - 9000, seed=600 + c)}
    chain = [("compressor", [1, 30, -20]), ("tone_stack", None), ("power_amp", "a"), ("power_amp", "b"), ("cabinet", None)]
    opts = {"fir_fused": 1, "fir_ahead_min_channels": 1}
    x = blocks(nch, 3, c0=20)
    res = {}
    for ahead in (False, True):
        ctx, h = make(pkg, nch, chain, irs, ahead, options=opts)
        res[ahead] = resident_calls(ctx, x, before + after, between=lambda c: action(c, h), at=before - 1)
        ctx.close()
    assert res[False][2] == 0
    # the calls behind the action start over: more than the first run alone, at most two separate runs of calls
    first, second = (expected_used(nch, 8, n) + expected_used(nch, 7, n) for n in (before, after))
    assert first < res[True][2] <= first + second, res[True][2]
    for b in range(before + after):
        assert np.array_equal(res[True][0][b], res[False][0][b]), "call %d" % b
    for e_on, e_off in zip(res[True][1], res[False][1]):
        assert np.array_equal(e_on, e_off)


def _data_calls(ctx, h):
    """calls on caller data only: a buffer made, written, read and freed, a level meter run"""
    nch = len(h)
    d = ctx.alloc(nch, FRAMES)
    d.upload(np.zeros((nch, FRAMES)))
    d.download()
    d.free()
    ctx.meter_configure(1)
    ctx.meter_process(np.zeros((1, FRAMES)), SR)
    return []


def test_calls_on_caller_data_keep_the_sums(pkg):
    """the host-buffer loop of an integration calls codecs, tuner, meters and copies between process calls: the sums stay usable"""
    nch, before, after = 8, 6, 6
    irs = {"a": lambda c: synth_ir(TAPS, seed=500 + c), "b": lambda c: synth_ir(TAPS - 9000, seed=600 + c)}
    chain = [("compressor", [1, 30, -20]), ("tone_stack", None), ("power_amp", "a"), ("power_amp", "b"), ("cabinet", None)]
    opts = {"fir_fused": 1, "fir_ahead_min_channels": 1}
    x = blocks(nch, 3, c0=20)
    res = {}
    for ahead in (False, True):
        ctx, h = make(pkg, nch, chain, irs, ahead, options=opts)
        res[ahead] = resident_calls(ctx, x, before + after, between=lambda c: _data_calls(c, h), at=before - 1)
        ctx.close()
    n = before + after
    assert res[True][2] == expected_used(nch, 8, n) + expected_used(nch, 7, n), res[True][2]
    for b in range(n):
        assert np.array_equal(res[True][0][b], res[False][0][b]), "call %d" % b


def test_host_buffer_calls_continue_the_sums(pkg):
    """gdg_process_staged back to back (the boundary's own path), two pcie groups of 256: bits and the device's count"""
    nch, calls = 512, 2 * T + 1
    irs = {"a": lambda c: synth_ir(TAPS, seed=5), "b": lambda c: synth_ir(TAPS, seed=6)}
    x = blocks(nch, calls, c0=1)
    res = {}
    for ahead in (False, True):
        ctx, _ = make(pkg, nch, BENCH, irs, ahead)
        outs = [ctx.process_staged(list(range(nch)), x[b], SR).copy() for b in range(calls)]
        ctx.synchronize()
        res[ahead] = (outs, ctx.get_option("stat_fir_ahead_sums_used"))
        ctx.close()
    assert res[False][1] == 0
    assert res[True][1] == expected_used(256, 8, calls) * 2 * 2, res[True][1]
    for b in range(calls):
        assert np.array_equal(res[True][0][b], res[False][0][b]), "call %d" % b
