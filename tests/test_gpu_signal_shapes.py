"""The signal as the input nobody pointed at: every unit type, in every build of the segment text, on the family of tests/signal_shapes.py --
above full scale, at the edge of the subnormal range, exact zeros and exact +-1.0, DC, a step, one non-zero sample -- and on a stream with ONE
non-finite sample.  The yardstick, the oracle on these signals, is checked on the CPU in test_signal_shapes_host.py.

Two bars per row and call, both the project's 1e-9 (north_star): rms(got - want) <= 1e-9 max(1, rms(want)), and, new here, per sample
max |got - want| <= 1e-9 max(1, max |want|) -- the RMS alone lets one wrong sample of a sparse output through, diluted by 1 / sqrt(N).
The tables the tests print are kept in profiles/parity_signal_shapes.txt (run with -s).

FOUND: no kernel was wrong; every row passes both bars in every build (worst 8.8e-12 RMS, 5.8e-10 per sample: fuzz [1, 100, 0, 30, 100, 0, 0]
on loud1000 at 48 kHz), and the NaNs of part (c) stand where the oracle has them.  One thing the bars do NOT see: both are absolute below a
reference of size 1, so on `tiny` and `subnormal` (outputs of 1e-11 and less out of every row but the signal generator) they catch a
non-finite or grossly wrong sample -- a scan table that meets 0 or a denormal and answers with NaN, inf or full-scale garbage -- and not a wrong
small value.  A relative bar for `tiny` is the open next step; the subnormal range has no meaningful relative bar.

Not held to the oracle, each with its reason:
  * signal_shapes.ILL_CONDITIONED (shape and finiteness only): empty, nothing of the family is ill-conditioned at these gains;
  * part (c), the two auto-yoy rows: the reference panics on a non-finite envelope (signal_shapes.POISON_DROPPED)."""
import numpy as np
import pytest

import test_gpu_os_tiles
import test_gpu_segf
import test_gpu_tile
from helpers import TOL_RMS, launches, package, rms, shapes, synth_ir
from signal_shapes import ILL_CONDITIONED, NAMES, PAIRS, POISON_AT, base_signal, key, oracle_row, row_channel, signals
from test_gpu_fuzz import reference_panics
from test_gpu_parity import UNIT_CASES
from test_signal_shapes_host import poison_rows

pytestmark = pytest.mark.gpu

TOL_PEAK = 1e-9         # the same 1e-9, per sample
SR_B, B, CALLS_B = PAIRS[0]


@pytest.fixture(scope="module")
def pkg():
    p = package()
    assert p.device_count() > 0, "no HIP device: the gpu tests must run on the GPU box"
    return p


def hold(got, want, frames, label, failures, where_finite=False):
    """Both bars per call of `frames` samples.  Returns (worst RMS, its call, worst peak error, its call).  where_finite: only samples at which
    both are finite are compared (part c)."""
    worst = (-1.0, -1, -1.0, -1)
    for call in range(got.size // frames):
        g, w = got[call * frames:(call + 1) * frames], want[call * frames:(call + 1) * frames]
        if where_finite:
            both = np.isfinite(g) & np.isfinite(w)
            g, w = g[both], w[both]
        elif not np.isfinite(g).all():
            failures.append("%s call %d: %d samples are not finite" % (label, call, int((~np.isfinite(g)).sum())))
            continue
        if not g.size:
            continue
        e_rms, e_peak = rms(g - w), float(np.max(np.abs(g - w)))
        if e_rms > worst[0]:
            worst = (e_rms, call) + worst[2:]
        if e_peak > worst[2]:
            worst = worst[:2] + (e_peak, call)
        if e_rms > TOL_RMS * max(1.0, rms(w)):
            failures.append("%s call %d: RMS %.3e (of %.3e)" % (label, call, e_rms, rms(w)))
        if e_peak > TOL_PEAK * max(1.0, float(np.max(np.abs(w)))):
            at = int(np.argmax(np.abs(g - w)))
            failures.append("%s call %d: peak error %.3e at its sample %d (largest |want| %.3e)" % (label, call, e_peak, at, float(np.max(np.abs(w)))))
    return worst


# ---- a. every row on every signal ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("sr,frames,calls", PAIRS)
def test_every_unit_case_on_every_signal(pkg, oracle, sr, frames, calls, name, capfd, monkeypatch):
    for unit, params in UNIT_CASES:
        for f, taps in ((2, 77), (4, 155)):
            assert not reference_panics(f * frames, taps)
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    n = frames * calls
    x = np.stack([signals(row_channel(k), n, sr, frames)[name] for k in range(len(UNIT_CASES))])
    want = np.stack([oracle_row(oracle, unit, params, x[k], [frames] * calls, sr) for k, (unit, params) in enumerate(UNIT_CASES)])
    ctx = pkg.Context(len(UNIT_CASES), frames)
    for k, (unit, params) in enumerate(UNIT_CASES):
        ctx.append_unit(k, unit, params=params)
    capfd.readouterr()
    got, ran = np.zeros_like(x), []
    for call in range(calls):
        out = ctx.process(np.ascontiguousarray(x[:, call * frames:(call + 1) * frames]), sr)
        ran.append({r["shape"] for r in launches(capfd.readouterr().err)})
        assert out.shape == (len(UNIT_CASES), frames), (call, out.shape)
        got[:, call * frames:(call + 1) * frames] = out
    ctx.close()
    failures, ill = [], 0
    top_rms, top_peak = (-1.0, -1, None), (-1.0, -1, None)
    for k, (unit, params) in enumerate(UNIT_CASES):
        label = "%s %s" % (unit, params)
        if key(unit, params) + (name, sr) in ILL_CONDITIONED:
            ill += 1
            if not np.isfinite(got[k]).all():
                failures.append(label + ": not finite")
            continue
        e_rms, c_rms, e_peak, c_peak = hold(got[k], want[k], frames, label, failures)
        if e_rms > top_rms[0]:
            top_rms = (e_rms, c_rms, label)
        if e_peak > top_peak[0]:
            top_peak = (e_peak, c_peak, label)
    print("\n[signal shapes] %6d Hz x %4d  %-20s RMS %.3e (call %d, %s)  peak %.3e (call %d, %s)  ill-conditioned, not held: %d" % (
        (sr, frames, name) + top_rms + top_peak + (ill,)))
    if frames == 8192:
        print("[signal shapes] %6d Hz x %4d  %-20s the calls ran %s" % (sr, frames, name, sorted(set().union(*ran))))
    assert not failures, "\n".join(failures)
    for shapes_ran in ran:
        assert shapes_ran, "no launch traced"
        if frames != 8192:
            assert shapes_ran == {"GENERAL"}, shapes_ran


# ---- b. the other builds of the segment text ------------------------------------------------------------------------------------------------
def family_rows(channels, n, rotate=0):
    """x [len(channels)][n] at 48 kHz: row i is signal NAMES[(i + rotate) % 13] made of synth_signal(channels[i]); and the names"""
    names = [NAMES[(i + rotate) % len(NAMES)] for i in range(len(channels))]
    return np.stack([signals(c, n, SR_B, B)[names[i]] for i, c in enumerate(channels)]), names


@pytest.mark.parametrize("rotate", range(len(NAMES)))
def test_the_two_per_cu_build_on_the_family(oracle, rotate, monkeypatch, capfd):
    """SEGF, forced on for 16 channels: the in-place units and the bench chain, channel c on signal (c + rotate) mod 13 -- over the thirteen
    cases every unit meets every signal.  Against the oracle at both bars, against the general kernel at 1e-12 max(1, max |want|)."""
    pkg = package()
    chains = [[u] for u in test_gpu_segf.FAST_UNITS] + [test_gpu_segf.BENCH_CHAIN]
    x, names = family_rows(list(range(len(chains))), CALLS_B * B, rotate)
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    monkeypatch.setenv("GDG_SEG_FAST_MIN", "0")
    ctx, refs = test_gpu_segf.build(pkg, oracle, chains)
    capfd.readouterr()
    fast, want = test_gpu_segf.stream(ctx, refs, x, SR_B, [B] * CALLS_B)
    ctx.close()
    ran_fast = shapes(capfd.readouterr().err)
    monkeypatch.setenv("GDG_SEG_FAST", "0")
    ctx, _ = test_gpu_segf.build(pkg, None, chains)
    ctx.set_option("seg_tile_max_channels", 0)          # sixteen channels: the defaults would put the frame on two workgroups (SEGT)
    general, _ = test_gpu_segf.stream(ctx, [None] * len(chains), x, SR_B, [B] * CALLS_B)
    ctx.close()
    ran_general = shapes(capfd.readouterr().err)
    failures, top = [], (-1.0, -1, -1.0, -1)
    for c, chain in enumerate(chains):
        label = "%s on %s" % (chain if len(chain) == 1 else "bench chain", names[c])
        w = hold(fast[c], want[c], B, label, failures)
        top = (max(top[0], w[0]), 0, max(top[2], w[2]), 0)
        apart = float(np.max(np.abs(fast[c] - general[c]))) if np.isfinite(general[c]).all() and np.isfinite(fast[c]).all() else float("inf")
        if not apart <= 1e-12 * max(1.0, float(np.max(np.abs(want[c])))):
            failures.append("%s: SEGF and the general kernel are %.3e apart" % (label, apart))
    print("\n[signal shapes] SEGF rotate %2d: worst RMS %.3e, worst peak %.3e; ran %s against %s" % (rotate, top[0], top[2], sorted(ran_fast), sorted(ran_general)))
    assert "SEGF" in ran_fast and not ran_fast & {"GENERAL", "GENERAL_AHEAD", "SEGT"}, ran_fast
    assert ran_general & {"GENERAL", "GENERAL_AHEAD"} and not ran_general & {"SEGF", "SEGT"}, ran_general
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("chain_name", sorted(test_gpu_tile.CHAINS))
def test_a_frame_on_two_workgroups_on_the_family(pkg, oracle, chain_name, monkeypatch, capfd):
    """SEGT: the 5-channel contexts of test_gpu_tile.py, three of them so that the thirteen signals pass five at a time.  Tiled and general runs
    bit for bit, EVERY channel against the oracle."""
    nch = 5
    chain = test_gpu_tile.CHAINS[chain_name]
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    failures, top = [], (-1.0, -1.0)
    for group in range(3):
        x, names = family_rows([c + 1 for c in range(nch)], CALLS_B * B, rotate=nch * group)
        outs, ran = {}, {}
        for tile in (False, True):
            ctx = test_gpu_tile.build(pkg, nch, chain, tile)
            capfd.readouterr()
            outs[tile] = test_gpu_tile.stream(ctx, x, SR_B, CALLS_B)
            ctx.close()
            ran[tile] = shapes(capfd.readouterr().err)
        assert "SEGT" in ran[True] and "SEGT" not in ran[False], ran
        for c in range(nch):
            if not np.array_equal(outs[True][c], outs[False][c]):
                failures.append("%s on %s: the tiled run does not have the general kernel's bits" % (chain_name, names[c]))
            ref = oracle.Chain()
            for uname, p in chain:
                if isinstance(p, str):
                    ref.append_unit(uname, fir=synth_ir(12000, seed=21 + 2 * c + (p == "b")))
                else:
                    ref.append_unit(uname, params=p)
            want = np.concatenate([ref.process(x[c, b * B:(b + 1) * B], SR_B) for b in range(CALLS_B)])
            w = hold(outs[True][c], want, B, "%s on %s" % (chain_name, names[c]), failures)
            top = (max(top[0], w[0]), max(top[1], w[2]))
    print("\n[signal shapes] SEGT %-22s worst RMS %.3e, worst peak %.3e" % (chain_name, top[0], top[1]))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("chain_name", sorted(test_gpu_os_tiles.CHAINS))
def test_the_oversampling_tiles_on_the_family(pkg, oracle, chain_name, monkeypatch, capfd):
    """The chains and the option of test_gpu_os_tiles.py, thirteen channels, one per signal: the tiles' bits are the in-segment unit's, and the
    oracle's samples at both bars."""
    nch = len(NAMES)
    chain = test_gpu_os_tiles.CHAINS[chain_name]
    x, names = family_rows([c + 1 for c in range(nch)], CALLS_B * B)
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    outs, ran = {}, {}
    for tiles in (False, True):
        ctx = test_gpu_os_tiles.build(pkg, nch, B, chain, tiles)
        capfd.readouterr()
        outs[tiles] = np.hstack([ctx.process(np.ascontiguousarray(x[:, b * B:(b + 1) * B]), SR_B) for b in range(CALLS_B)])
        ctx.close()
        ran[tiles] = shapes(capfd.readouterr().err) & {"OS_TILES", "OS_TILES_PREFIX"}
    assert ran[True] and not ran[False], ran
    failures, top = [], (-1.0, -1.0)
    for c in range(nch):
        if not np.array_equal(outs[True][c], outs[False][c]):
            failures.append("%s on %s: the tiles do not have the in-segment unit's bits" % (chain_name, names[c]))
        ref = oracle.Chain()
        for uname, p in chain:
            if p == "ir":
                ref.append_unit(uname, fir=synth_ir(9000, seed=3 + c))
            else:
                ref.append_unit(uname, params=p)
        want = np.concatenate([ref.process(x[c, b * B:(b + 1) * B], SR_B) for b in range(CALLS_B)])
        w = hold(outs[True][c], want, B, "%s on %s" % (chain_name, names[c]), failures)
        top = (max(top[0], w[0]), max(top[1], w[2]))
    print("\n[signal shapes] OS tiles %-24s worst RMS %.3e, worst peak %.3e; ran %s" % (chain_name, top[0], top[1], sorted(ran[True])))
    assert not failures, "\n".join(failures)


# ---- c. one non-finite sample ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_one_non_finite_sample_stays_where_the_reference_keeps_it(pkg, oracle, poison, monkeypatch, capfd):
    """Channel 2 j: row j of the time-domain, causal rows with the poisoned sample; channel 2 j + 1: the same row, clean.  Against a run of the
    same context with 0.0 in the sample's place: the clean channels and everything before the sample keep their bits; from the sample on the
    NaNs are where the oracle has them, and where both are finite both bars hold."""
    sr, frames, calls = PAIRS[1]
    n, at = frames * calls, frames + POISON_AT
    rows = poison_rows()
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")

    def inputs(value):
        x = np.stack([base_signal(row_channel(k), n, sr).copy() for k in rows for _ in range(2)])
        x[:, at] = 0.0
        x[0::2, at] = value
        return x

    def run(x):
        ctx = pkg.Context(2 * len(rows), frames)
        for j, k in enumerate(rows):
            for c in (2 * j, 2 * j + 1):
                ctx.append_unit(c, UNIT_CASES[k][0], params=UNIT_CASES[k][1])
        capfd.readouterr()
        got = np.hstack([ctx.process(np.ascontiguousarray(x[:, b * frames:(b + 1) * frames]), sr) for b in range(calls)])
        ctx.close()
        assert shapes(capfd.readouterr().err) == {"GENERAL"}
        assert got.shape == x.shape
        return got

    x = inputs(poison)
    clean, got = run(inputs(0.0)), run(x)
    assert np.isfinite(clean).all()
    failures, nans = [], 0
    for j, k in enumerate(rows):
        unit, params = UNIT_CASES[k]
        label = "%s %s" % (unit, params)
        if not np.array_equal(got[2 * j + 1], clean[2 * j + 1]):
            failures.append("%s: the clean channel beside the poisoned one changed" % label)
        if not np.array_equal(got[2 * j, :at], clean[2 * j, :at]):
            first = int(np.argmax(got[2 * j, :at] != clean[2 * j, :at]))
            failures.append("%s: a sample BEFORE the poisoned one changed, first at %d of %d" % (label, first, at))
        want = oracle_row(oracle, unit, params, x[2 * j], [frames] * calls, sr)
        if not np.array_equal(np.isnan(got[2 * j]), np.isnan(want)):
            differ = np.nonzero(np.isnan(got[2 * j]) != np.isnan(want))[0]
            failures.append("%s: NaN at %d samples here, at %d in the oracle; they differ at %d samples, first %d" % (
                label, int(np.isnan(got[2 * j]).sum()), int(np.isnan(want).sum()), differ.size, int(differ[0])))
        nans += int(np.isnan(want).sum())
        hold(got[2 * j], want, frames, label, failures, where_finite=True)
    print("\n[signal shapes] %s at sample %d of %d rows: %d NaN samples in the oracle's outputs; failures %d" % (poison, at, len(rows), nans, len(failures)))
    assert not failures, "\n".join(failures)
