"""Frame length as the input nobody pointed at: every unit type at short, odd and ragged frames (tests/frame_lengths.py), power amps below 64
frames, and what the device-resident entry points do with a pointer that is not 16-byte aligned.  The yardstick -- the oracle at these
lengths -- is checked on the CPU in test_frame_lengths_host.py.  Tolerance: 1e-9 RMS per call and channel (north_star); at N = 1 that is the
absolute error.  The tables the tests print are kept in profiles/parity_frame_lengths.txt (run with -s).

FOUND by (a): the ten 2x / 4x oversampled shaper and fuzz rows were 0.2 to 0.9 RMS away from the oracle at 7 (22050 Hz), 10 (48 kHz) and 13
(192 kHz) calls of the schedule and within 1e-13 at all others.  Those calls are exactly the ones at which the REFERENCE has no output: the
unit's decimator runs filter.Process on the F N oversampled samples (oversampling/oversampling.go:149-150), and that panics on a slice bound
when F N is not a power of two and a block of nextpow2(taps) samples starts beyond it (filter/filter.go:370-382, :443-453) -- N = 1025, 2049,
3000, 4097 and most ring capacities (frame_lengths.decimator_pair, test_gpu_fuzz.reference_panics; the list is pinned on the CPU in
test_frame_lengths_host.py).  The oracle stops in mid-frame there (oracle/filter.c: -3), so its samples are no yardstick; the kernels carry on
with the time-domain filter.  Such a (row, call) is held to shape and finiteness only and counted in the table ("no ref"); every other call of
the same row, the ones right behind a panicking call included, is held to the oracle as usual.  The library does not refuse these calls
as it refuses the power amps' panicking pairs (api_plan.cpp prepare_fir): DESIGN.md section 3."""
import numpy as np
import pytest

from frame_lengths import MAX_FRAMES, RATES, decimator_pair, schedule
from helpers import TOL_RMS, ChainPair, launches, package, rms, synth_ir, synth_signal
from test_gpu_fuzz import reference_panics
from test_gpu_parity import UNIT_CASES, full_chain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = package()
    assert p.device_count() > 0, "no HIP device: the gpu tests must run on the GPU box"
    return p


_streams = {}


def oracle_stream(oracle, sr):
    """(x, want) [len(UNIT_CASES)][total]: case k on row k, input synth_signal(7 k + 3), cut by schedule(sr); made once per rate and shared"""
    if sr not in _streams:
        cuts = schedule(sr)
        total = sum(cuts)
        x = np.stack([synth_signal(7 * k + 3, total, sr) for k in range(len(UNIT_CASES))])
        want = np.zeros_like(x)
        for k, (unit, params) in enumerate(UNIT_CASES):
            ch = oracle.Chain()
            ch.append_unit(unit, params=params)
            pos = 0
            for n in cuts:
                want[k, pos:pos + n] = ch.process(x[k, pos:pos + n], sr)
                pos += n
        x.setflags(write=False)
        want.setflags(write=False)
        _streams[sr] = (x, want)
    return _streams[sr]


def run_schedule(pkg, oracle, sr, rows, capfd, option=None):
    """The rows (indices into UNIT_CASES) of the stream through schedule(sr), one ctx.process per entry.  Returns (failures, table lines, the
    shapes every call ran: [(N, set)]).  A call on which the reference panics inside the row's decimator has no reference (module docstring)."""
    x, want = oracle_stream(oracle, sr)
    cuts = schedule(sr)
    ctx = pkg.Context(len(rows), MAX_FRAMES)
    if option:
        ctx.set_option(*option)
    for c, k in enumerate(rows):
        ctx.append_unit(c, UNIT_CASES[k][0], params=UNIT_CASES[k][1])
    capfd.readouterr()
    failures, ran = [], []
    worst = [(-1.0, -1, 0)] * len(rows)            # (RMS, call, N)
    no_ref = [0] * len(rows)
    pos = 0
    for call, n in enumerate(cuts):
        got = ctx.process(np.ascontiguousarray(x[rows, pos:pos + n]), sr)
        ran.append((n, {r["shape"] for r in launches(capfd.readouterr().err)}))
        if got.shape != (len(rows), n):
            failures.append("call %d (N = %d): shape %s" % (call, n, got.shape))
            break
        for c, k in enumerate(rows):
            finite = bool(np.isfinite(got[c]).all())
            pair = decimator_pair(UNIT_CASES[k][0], UNIT_CASES[k][1], n)
            if finite and pair and reference_panics(*pair):
                no_ref[c] += 1
                continue
            err = rms(got[c] - want[k, pos:pos + n]) if finite else float("inf")
            if err > worst[c][0]:
                worst[c] = (err, call, n)
            if not finite or err > TOL_RMS:
                failures.append("call %d (N = %d) %s %s: RMS %.3e" % (call, n, UNIT_CASES[k][0], UNIT_CASES[k][1], err))
        pos += n
    ctx.close()
    table = ["%-18s %-32s call %2d  N %4d  RMS %.3e%s" % (UNIT_CASES[k][0], UNIT_CASES[k][1], worst[c][1], worst[c][2], worst[c][0],
                                                            "  (no ref: %d calls)" % no_ref[c] if no_ref[c] else "") for c, k in enumerate(rows)]
    return failures, table, ran


# ---- a. every unit type through the schedule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_every_unit_case_through_the_schedule(pkg, oracle, sr, capfd, monkeypatch):
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    failures, table, ran = run_schedule(pkg, oracle, sr, list(range(len(UNIT_CASES))), capfd)
    # (behind the last readouterr: what is printed from here on reaches the report of a failure, or the terminal with -s)
    print("\n[frame lengths] %d Hz, %d calls, %d samples; per case the worst call" % (sr, len(ran), sum(n for n, _ in ran)))
    print("\n".join(table))
    print("[frame lengths] %d Hz: the 8192-sample calls ran %s" % (sr, [sorted(s) for n, s in ran if n == MAX_FRAMES]))
    assert not failures, "\n".join(failures)
    for n, shapes_ran in ran:
        if n != MAX_FRAMES:
            assert shapes_ran == {"GENERAL"}, (n, shapes_ran)
        else:
            assert shapes_ran, "no launch traced"


# ---- b. a ragged frame on every build's neighbour --------------------------------------------------------------------------------------
FEW = [0, 1, 2, UNIT_CASES.index(("tone_stack", None)), UNIT_CASES.index(("chorus", None))]


def test_few_channels_between_odd_frames_in_the_shape_the_defaults_pick(pkg, oracle, capfd, monkeypatch):
    """Three compressors, a tone stack and a chorus, five channels: with the defaults their 8192-sample call is split over two workgroups per
    channel (SEGT, seg.hip built with -DSEG_TILE), with seg_tile_max_channels = 0 it runs the general kernel.  Both legs: the 48 kHz stream of
    (a), so the tiled call sits between an 8191 and a 7, its state written by the general kernel and read by it again."""
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    legs = {}
    for name, option in (("default", None), ("seg_tile_max_channels = 0", ("seg_tile_max_channels", 0))):
        legs[name] = run_schedule(pkg, oracle, 48000, FEW, capfd, option)
    at_full = {name: [sorted(s) for n, s in ran if n == MAX_FRAMES] for name, (_, _, ran) in legs.items()}
    for name, (failures, table, ran) in legs.items():
        print("\n[frame lengths] few channels, %s: the 8192-sample calls ran %s" % (name, at_full[name]))
        print("\n".join(table))
    for name, (failures, table, ran) in legs.items():
        assert not failures, name + "\n" + "\n".join(failures)
        for n, shapes_ran in ran:
            if n != MAX_FRAMES:
                assert shapes_ran == {"GENERAL"}, (name, n, shapes_ran)
    assert at_full["default"] != at_full["seg_tile_max_channels = 0"], at_full


# ---- c. power amps below 64 frames ------------------------------------------------------------------------------------------------------
def _fir_stream(pkg, oracle, sizes, taps, max_frames):
    sr = 48000
    for n in set(sizes):
        assert not reference_panics(n, taps), (n, taps)
    ctx = pkg.Context(2, max_frames)
    h = [synth_ir(taps, seed=4242 + c) * (3.0 if c else 1.0) for c in range(2)]         # channel 1 is driven into the clip
    pairs = []
    for c in range(2):
        p = ChainPair(ctx, c, oracle)
        p.append("power_amp", fir=h[c])
        pairs.append(p)
    x = np.stack([synth_signal(c, sum(sizes), sr) for c in range(2)])
    got, want = np.zeros_like(x), np.zeros_like(x)
    pos = 0
    for n in sizes:
        blk = np.ascontiguousarray(x[:, pos:pos + n])
        out = ctx.process(blk, sr)
        assert out.shape == (2, n) and np.isfinite(out).all(), (pos, n)
        got[:, pos:pos + n] = out
        for c in range(2):
            want[c, pos:pos + n] = pairs[c].ref.process(blk[c], sr)
        pos += n
    ctx.close()
    worst_rms, worst_rel = 0.0, 0.0
    for c in range(2):
        direct = np.clip(np.convolve(x[c], h[c])[:x.shape[1]], -1.0, 1.0)
        worst_rms = max(worst_rms, rms(got[c] - want[c]))
        worst_rel = max(worst_rel, float(np.max(np.abs(got[c] - direct)) / np.max(np.abs(direct))))
    return worst_rms, worst_rel


@pytest.mark.parametrize("frames,taps", [(1, 1), (1, 5), (2, 3), (4, 1), (8, 77), (16, 200), (32, 1000), (32, 33)])
def test_power_amp_below_64_frames(pkg, oracle, frames, taps):
    worst_rms, worst_rel = _fir_stream(pkg, oracle, [frames] * 40, taps, frames)
    print("\n[frame lengths] power amp %2d frames x 40, %4d taps: RMS vs oracle %.3e, max-abs vs numpy.convolve / largest output %.3e" % (
        frames, taps, worst_rms, worst_rel))
    assert worst_rms <= TOL_RMS
    assert worst_rel <= 1e-12


def test_power_amp_through_changing_short_frames(pkg, oracle):
    """One context, 200 taps: the delay line is re-partitioned at every change of the frame length, down to one sample and back."""
    sizes = [32, 32, 8, 8, 1, 1, 16, 64, 2, 32]
    worst_rms, worst_rel = _fir_stream(pkg, oracle, sizes, 200, 64)
    print("\n[frame lengths] power amp %s, 200 taps: RMS vs oracle %.3e, max-abs vs numpy.convolve / largest output %.3e" % (sizes, worst_rms, worst_rel))
    assert worst_rms <= TOL_RMS
    assert worst_rel <= 1e-12


# ---- d. device pointers that are not 16-byte aligned -------------------------------------------------------------------------------------
def _device_context(pkg):
    """Four channels: the full chain (8192 taps) on two, compressor to reverb without amps on two"""
    ctx = pkg.Context(4, MAX_FRAMES)

    class Direct:              # full_chain() speaks to a ChainPair
        def __init__(self, c):
            self.c = c

        def append(self, unit, params=None, fir=None):
            ctx.append_unit(self.c, unit, params=params, fir=fir)
    for c in range(2):
        full_chain(Direct(c), 0, synth_ir(8192, seed=4242 + c))
    for c in range(2, 4):
        for unit, params in (("compressor", [1, 30, -20]), ("overdrive", [0, 20, 100, 0, 1, 1]), ("tone_stack", None), ("chorus", None),
                             ("cabinet", None), ("reverb", [50])):
            ctx.append_unit(c, unit, params=params)
    return ctx


def test_misaligned_device_pointers_are_refused_and_change_nothing(pkg):
    """The text decides (include/gdg.h, api_process.cpp check_pair_alignment): the convolution's first pass reads the caller's frame as
    16-byte pairs (fir.hip: gload of a cplx at bsrc + 2 e in every forward kernel), its last pass stores pairs to dst, and the oversampling
    tiles store pairs to dst and load them from the compressor prefix's src (seg.hip os_tiles_kernel) -- none of them looks at the pointer;
    only seg_frame does.  So a pointer offset by one double, or an odd row stride, is NOT run: both entry points refuse it with
    GDG_ERR_INVALID and name what is wrong.  A refused call launches nothing: the stream around it has the bits of a stream without it."""
    sr, B, blocks, W = 48000, MAX_FRAMES, 8, 4
    x = np.stack([synth_signal(3 * c + 1, blocks * B, sr) for c in range(4)])

    def run(provoke):
        ctx = _device_context(pkg)
        ctx.set_window(W)
        d_in, d_out = ctx.alloc(4, blocks * B), ctx.alloc(4, blocks * B)
        d_blk_in, d_blk_out = ctx.alloc(4, B), ctx.alloc(4, B)
        d_in.upload(x)
        out = []
        for b in range(4):                                 # frames 0 .. 3 one by one through gdg_process_device
            d_blk_in.upload(np.ascontiguousarray(x[:, b * B:(b + 1) * B]))
            if provoke and b in (1, 3):                    # (a refused call reads and writes nothing: the offsets need no room behind the buffers)
                for frames in (8192, 4096, 1000):
                    for off_in, off_out, name in ((8, 0, "d_in"), (0, 8, "d_out"), (8, 8, "d_in")):
                        with pytest.raises(pkg.GdgError, match=name + " .* is not 16-byte aligned") as e:
                            ctx.process_device(d_blk_in.ptr + off_in, d_blk_out.ptr + off_out, frames, sr)
                        assert e.value.code == pkg.GDG_ERR_INVALID
            ctx.process_device(d_blk_in, d_blk_out, B, sr)
            out.append(d_blk_out.download())
        at = 8 * 4 * B                                     # frames 4 .. 7 as one window over the rows of the whole stream
        if provoke:
            with pytest.raises(pkg.GdgError, match="row stride %d is odd" % (blocks * B + 1)) as e:
                ctx.process_window_device(d_in.ptr + at, d_out.ptr + at, blocks * B + 1, W, sr)
            assert e.value.code == pkg.GDG_ERR_INVALID
            for off_in, off_out, name in ((8, 0, "d_in"), (0, 8, "d_out"), (8, 8, "d_in")):
                with pytest.raises(pkg.GdgError, match=name + " .* is not 16-byte aligned") as e:
                    ctx.process_window_device(d_in.ptr + at + off_in, d_out.ptr + at + off_out, blocks * B, W, sr)
                assert e.value.code == pkg.GDG_ERR_INVALID
        ctx.process_window_device(d_in.ptr + at, d_out.ptr + at, blocks * B, W, sr)
        got = d_out.download()[:, 4 * B:]
        ctx.close()
        return np.hstack(out + [got])

    plain, provoked = run(False), run(True)
    assert np.isfinite(plain).all() and np.abs(plain).max() > 0.01
    assert np.array_equal(plain, provoked), "a refused call changed the stream: max diff %.3e" % np.max(np.abs(plain - provoked))
