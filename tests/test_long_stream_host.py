"""The reference's conditioning on the parity gate's own stream ("What's weak", first bullet).

bench.py's in-run gate follows global channels 0 / 256 / 511 through `bench.CHAIN` at 192 kHz, 8192-sample frames, the calls walking round
robin over the 4 blocks of `bench.synth_blocks` -- block 3 is followed by block 0, a real discontinuity of the input every fourth call.  With
the driver's flags the gate compares calls 171-173 and read 7.7e-11 from round 6 on; with the default flags it compares calls 226-228 and read
7.7e-15 (one sample of the device's chorus at call 133; the oracle itself is conditioned to 1e-12 everywhere, as below).

This file says how far the ORACLE moves on that stream (176 calls, every prefix 1..8 of the chain, 8192-tap IRs) under two perturbations:
  (a) every exp / sin / cos / atan / pow / log10 / log2 result moved by a seeded -2 .. +2 ulp (oracle/libm_jitter.h), seeds 1, 2 and 7;
  (b) every input sample moved by a seeded -2 .. +2 ulp.
Every block of every prefix must stay under TOL_RMS / 10, the bound tests/test_libm_sensitivity.py uses for the same question.  The larger of
the two per prefix and block, over the three channels, is `ref_spread()[prefix - 1][block]`: what tests/test_gpu_long_stream.py measures the
device's distance from the oracle against.

A chain is its units applied one after the other (oracle/chain.c), so one pass through eight one-unit chains gives all eight prefixes; the
first test pins that against a single eight-unit chain."""
import functools
import sys

import numpy as np
import pytest

import __graft_entry__ as entry

sys.path.insert(0, entry.ROOT)
from helpers import TOL_RMS  # noqa: E402
import bench  # noqa: E402  (read-only: CHAIN, synth_blocks, ir_for)

SR, FRAMES, CALLS, TAPS = 192000, 8192, 176, 8192
CHANNELS = (0, 256, 511)
JITTER_SEEDS = (1, 2, 7)
INPUT_SEED = 20260
N_UNITS = len(bench.CHAIN)


@functools.lru_cache(maxsize=None)
def input_blocks(g):
    """[4][frames]: the gate's input blocks of global channel g."""
    return np.ascontiguousarray(bench.synth_blocks(1, FRAMES, SR, channel0=g)[:, 0, :])


@functools.lru_cache(maxsize=None)
def irs(g, taps):
    return {"cab": bench.ir_for("cab", g, taps), "rev": bench.ir_for("rev", g, taps)}


def unit_chains(orc, g, taps):
    """bench.CHAIN for global channel g as eight one-unit oracle chains."""
    chains = []
    for name, p in bench.CHAIN:
        ch = orc.Chain()
        if isinstance(p, str):
            ch.append_unit(name, fir=irs(g, taps)[p])
        else:
            ch.append_unit(name, params=p)
        chains.append(ch)
    return chains


def prefix_stream(orc, g, taps=TAPS, calls=CALLS, blocks=None, keep=None):
    """The oracle over `calls` round-robin calls: out[k][b] = output of prefix k of bench.CHAIN on call b (out[0] = the input).
    keep: only these prefixes are stored (the others are None)."""
    blocks = input_blocks(g) if blocks is None else blocks
    chains = unit_chains(orc, g, taps)
    keep = range(N_UNITS + 1) if keep is None else keep
    out = [np.empty((calls, FRAMES)) if k in keep else None for k in range(N_UNITS + 1)]
    for b in range(calls):
        y = blocks[b % len(blocks)]
        for k in range(N_UNITS + 1):
            if k > 0:
                y = chains[k - 1].process(y, SR)
            if out[k] is not None:
                out[k][b] = y
    del chains
    return out


def moved_inputs(g):
    """The input blocks with every sample moved by a seeded -2 .. +2 ulp."""
    x = input_blocks(g)
    k = np.random.default_rng(INPUT_SEED + g).integers(-2, 3, size=x.shape)
    return x + k * np.spacing(np.abs(x))


def block_rms(a, b):
    """[prefixes][calls]: per-block RMS distance of two prefix_stream results, prefixes 1..8."""
    return np.array([np.sqrt(np.mean((a[k] - b[k]) ** 2, axis=1)) for k in range(1, N_UNITS + 1)])


def _oracle():
    orc = entry.load_oracle()
    orc.build()
    orc.build(jitter=True)
    return orc


@functools.lru_cache(maxsize=None)
def plain_stream(g):
    """The plain oracle's prefix_stream for global channel g (shared by the two modules, never changed)."""
    out = prefix_stream(_oracle(), g)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def spreads(g):
    """(spread_a, spread_b), each [prefixes][calls], for global channel g."""
    orc = _oracle()
    plain = plain_stream(g)
    a = np.zeros((N_UNITS, CALLS))
    for seed in JITTER_SEEDS:
        with orc.jittered(seed):
            moved = prefix_stream(orc, g)
            a = np.maximum(a, block_rms(plain, moved))
            del moved
    b = block_rms(plain, prefix_stream(orc, g, blocks=moved_inputs(g)))
    return a, b


@functools.lru_cache(maxsize=None)
def ref_spread():
    """[prefixes][calls]: the larger of the two spreads over the three channels -- the reference's own error on this stream."""
    return np.max([np.maximum(*spreads(g)) for g in CHANNELS], axis=0)


def bound(prefix):
    """What a device-to-oracle distance of `prefix` (1..8) is held to: 10 x the worst block of ref_spread, floor 1e-15 (prefixes without a
    libm call have spread 0).  One decade for FFT and scan association, which neither perturbation models."""
    return max(10.0 * float(ref_spread()[prefix - 1].max()), 1e-15)


def test_one_unit_chains_are_the_chain():
    orc = _oracle()
    whole = orc.Chain()
    for name, p in bench.CHAIN:
        if isinstance(p, str):
            whole.append_unit(name, fir=irs(0, TAPS)[p])
        else:
            whole.append_unit(name, params=p)
    x = input_blocks(0)
    got = prefix_stream(orc, 0, calls=6, keep=(N_UNITS,))[N_UNITS]
    for b in range(6):
        np.testing.assert_array_equal(got[b], whole.process(x[b % 4], SR))


def test_the_input_perturbation_perturbs():
    for g in CHANNELS:
        x, m = input_blocks(g), moved_inputs(g)
        assert 0.0 < np.abs(m - x).max() <= 2 * np.spacing(np.abs(x)).max()
        assert np.count_nonzero(m != x) > 0.7 * x.size


@pytest.mark.parametrize("g", CHANNELS)
def test_every_block_of_every_prefix_is_conditioned(g):
    a, b = spreads(g)
    print("channel %d: worst block per prefix, (a) libm jitter seeds %s / (b) inputs moved by +-2 ulp" % (g, list(JITTER_SEEDS)))
    for k in range(N_UNITS):
        print("  prefix %d (.. %-10s)  (a) %.3e at block %3d   (b) %.3e at block %3d"
              % (k + 1, bench.CHAIN[k][0], a[k].max(), int(a[k].argmax()), b[k].max(), int(b[k].argmax())))
    assert a.max() <= TOL_RMS / 10, ("libm jitter", np.unravel_index(a.argmax(), a.shape), a.max())
    assert b.max() <= TOL_RMS / 10, ("input perturbation", np.unravel_index(b.argmax(), b.shape), b.max())


def test_ref_spread_is_shared_and_complete():
    r = ref_spread()
    assert r.shape == (N_UNITS, CALLS) and np.isfinite(r).all()
    assert r is ref_spread()
    assert bound(N_UNITS) <= TOL_RMS            # the x10 rule never asks less than the parity bar
