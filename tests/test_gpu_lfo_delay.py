"""Chorus, flanger and phaser on streams that land on WHOLE delays (tests/lfo_delay_ref.py finds them, tests/test_lfo_delay_host.py checks the
expectation on the CPU).  At a whole delay the reference counts the delayed sample twice; a kernel whose LFO is a rotated sincos is ~1e-16 off
and interpolates instead, which moves that output sample by the wet mix times the input (0.125 and more on these inputs).

Every leg runs a two-channel context: channel 1 carries the case, channel 0 the same unit at lfo_delay_ref.QUIET (a setting away from the
whole delays), so a whole delay sits in some lanes of a wave beside lanes without one.  Per case:

  - every block of channel 1 within TOL_RMS of the oracle (RMS; the fragile hits' samples are left out of it, they have their own leg);
  - at every robust hit |device - oracle| <= TOL_RMS at that very sample;
  - at every fragile hit (the reference's own answer depends on its libm there) the device's sample is within TOL_RMS of the restatement's
    value for one of the ulp offsets -2 .. +2 of that hit's sine;
  - channel 0 within TOL_RMS of the oracle; everything finite.

The chorus's near-whole branch is one text in seg.hip (unit_chorus), compiled three times (the general, the two-per-CU and the tile build, which
differ in the LFO's schedule and the tile's offset), and runs in four shapes; the 8192-frame chorus cases run in each, confirmed from the GDG_PLAN_TRACE=2 lines: SEGT (the defaults), GENERAL (seg_tile_max_channels = 0),
SEGF (seg_two_per_cu_min_channels = 2; segf_unit_ok holds for the chorus at every rate) and WAVE (windows of 4, also bit for bit against
the per-frame calls).  The flanger and the phaser run in the general kernel only; one flanger case also runs in windows.

Each leg prints its table: case, hit, delay, device - oracle."""
import functools

import numpy as np
import pytest

import __graft_entry__ as entry
from helpers import TOL_RMS, launches
import lfo_delay_ref as ref
import test_lfo_delay_host as host

pytestmark = pytest.mark.gpu

CASES, IDS = host.CASES, host.IDS
CHORUS_8192 = [k for k, c in enumerate(CASES) if c.unit == "chorus" and c.frames == 8192]
OTHERS = [k for k in range(len(CASES)) if k not in CHORUS_8192]
SHAPES = {"SEGT": {}, "GENERAL": {"seg_tile_max_channels": 0}, "SEGF": {"seg_two_per_cu_min_channels": 2}}
WINDOW = 4
WINDOW_FLANGER = next(k for k, c in enumerate(CASES) if c.unit == "flanger" and c.frames == 8192 and c.calls <= 100)


@pytest.fixture(scope="module")
def pkg():
    return entry.load_package()


@functools.lru_cache(maxsize=None)
def quiet_stream(k):
    """the oracle's stream of channel 0 of case k's context"""
    c = CASES[k]
    orc = entry.load_oracle()
    orc.build()
    out = host.oracle_blocks(orc, c.unit, ref.QUIET[c.unit], c.sr, host.case_inputs(k), c.calls)
    out.setflags(write=False)
    return out


def make_context(pkg, k, options):
    c = CASES[k]
    ctx = pkg.Context(2, c.frames)
    for key, v in options.items():
        ctx.set_option(key, v)
    ctx.append_unit(0, c.unit, params=ref.QUIET[c.unit])
    ctx.append_unit(1, c.unit, params=c.params)
    return ctx


def run_frames(pkg, k, options, capfd, monkeypatch):
    """([2][calls][frames], the launch shapes that ran): one process() per call"""
    c = CASES[k]
    x = host.case_inputs(k)
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    ctx = make_context(pkg, k, options)
    capfd.readouterr()
    out = np.empty((2, c.calls, c.frames))
    for b in range(c.calls):
        blk = x[b % len(x)]
        out[:, b, :] = ctx.process(np.stack([blk, blk]), c.sr)
    ctx.close()
    return out, {r["shape"] for r in launches(capfd.readouterr().err)}


def run_windows(pkg, k, capfd, monkeypatch):
    """the same stream in windows of WINDOW frames (the last one shorter)"""
    c = CASES[k]
    x = host.case_inputs(k)
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    ctx = make_context(pkg, k, {})
    ctx.set_window(WINDOW)
    n = c.calls * c.frames
    row = np.concatenate([x[b % len(x)] for b in range(c.calls)])
    d_in, d_out = ctx.alloc(2, n), ctx.alloc(2, n)
    d_in.upload(np.stack([row, row]))
    capfd.readouterr()
    b, ran = 0, set()
    while b < c.calls:
        w = WINDOW
        while w > c.calls - b:                     # the stream's tail: a window holds 1, 2, 4, 8 or 16 frames
            w //= 2
        ctx.process_window_device(d_in.ptr + 8 * b * c.frames, d_out.ptr + 8 * b * c.frames, n, w, c.sr)
        ctx.synchronize()
        shapes = {r["shape"] for r in launches(capfd.readouterr().err)}
        if w > 1:                                  # (a window of one frame is a per-frame call and takes that call's shape)
            ran |= shapes
        b += w
    out = d_out.download().reshape(2, c.calls, c.frames)
    ctx.close()
    return out, ran


def block_rms(d):
    return np.sqrt(np.mean(d * d, axis=1))


def check(k, got, leg):
    c = CASES[k]
    want = host.oracle_stream(k)
    hits = host.case_hits(k)
    lines, bad = [], []
    for h in hits:
        dev = got[1, h.call, h.sample]
        if h.robust:
            err = dev - want[h.call, h.sample]
            kind = "robust"
        else:
            alts = [ref.stream(c.unit, c.params, c.sr, c.frames, host.case_inputs(k).tolist(), h.call + 1, first=h.call,
                               offsets={(h.call, h.sample, h.lfo): o}, samples=[h.sample])[0][h.sample] for o in ref.ULP_OFFSETS]
            err = min((dev - a for a in alts), key=abs)
            kind = "fragile"
        lines.append("%-34s %-8s call %3d sample %4d lfo %d  delay %4d  %-7s device - %s %+.3e"
                     % (IDS[k], leg, h.call, h.sample, h.lfo, h.delay, kind, "oracle" if h.robust else "nearest of 5 answers", err))
        if not abs(err) <= TOL_RMS:
            bad.append((h, float(err)))
    d = got[1] - want
    for h in hits:
        if not h.robust:
            d[h.call, h.sample] = 0.0
    rms1 = block_rms(d)
    rms0 = block_rms(got[0] - quiet_stream(k))
    print("\n".join(lines))
    print("%-34s %-8s worst block RMS: channel 1 %.3e (block %d), channel 0 %.3e; hits missed: %d of %d"
          % (IDS[k], leg, rms1.max(), int(rms1.argmax()), rms0.max(), len(bad), len(hits)))
    assert np.isfinite(got).all()
    assert not bad, bad[:8]
    assert rms1.max() <= TOL_RMS, (int(rms1.argmax()), float(rms1.max()))
    assert rms0.max() <= TOL_RMS, (int(rms0.argmax()), float(rms0.max()))


@functools.lru_cache(maxsize=None)
def _per_frame_cache():
    return {}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("k", CHORUS_8192, ids=[IDS[k] for k in CHORUS_8192])
def test_chorus_whole_delays_in_every_per_frame_shape(pkg, capfd, monkeypatch, k, shape):
    got, ran = run_frames(pkg, k, SHAPES[shape], capfd, monkeypatch)
    assert ran == {shape}, ran
    if shape == "SEGT":
        _per_frame_cache()[k] = got
    check(k, got, shape)


@pytest.mark.parametrize("k", CHORUS_8192 + [WINDOW_FLANGER], ids=[IDS[k] for k in CHORUS_8192 + [WINDOW_FLANGER]])
def test_whole_delays_in_windows(pkg, capfd, monkeypatch, k):
    got, ran = run_windows(pkg, k, capfd, monkeypatch)
    assert ran == {"WAVE"}, ran
    frames = _per_frame_cache().get(k)
    if frames is None:
        frames = run_frames(pkg, k, {}, capfd, monkeypatch)[0]
    differ = [b for b in range(CASES[k].calls) if not np.array_equal(got[:, b], frames[:, b])]
    check(k, got, "WAVE")
    assert not differ, (differ[:8], float(np.abs(got - frames).max()))


@pytest.mark.parametrize("k", OTHERS, ids=[IDS[k] for k in OTHERS])
def test_whole_delays_of_flanger_phaser_and_the_odd_frame_chorus(pkg, capfd, monkeypatch, k):
    got, ran = run_frames(pkg, k, {}, capfd, monkeypatch)
    assert ran == {"GENERAL"}, ran
    if k == WINDOW_FLANGER:
        _per_frame_cache()[k] = got
    check(k, got, "GENERAL")
