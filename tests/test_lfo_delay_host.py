"""Whole-sample delays of the chorus, the flanger and the phaser: the expectation the GPU legs (tests/test_gpu_lfo_delay.py) hold the kernels
to, checked on the CPU first.

tests/lfo_delay_ref.py restates the three units in plain Python floats and finds the taps whose delay is a whole number of samples (the
reference counts the delayed sample twice there).  This module checks, without a GPU,

  - that the restatement and the oracle agree.  They agree BIT FOR BIT on every case (same glibc sin / fmod, the oracle is built with
    -ffp-contract=off), so the leg asserts equality and not the 1e-12 of the hand-calculated cases.  Streams of more than 1.1 M samples are
    restated from two calls in front of the case's first listed hit (the calls before only leave their state -- the phase and the delay
    buffer -- which the restated calls then depend on); shorter ones from call 0;
  - that the finder returns the hits the case table lists, every case holds at least two robust, sensitive hits besides sample 0 of call 0,
    and fragile hits are at most half of a case's hits;
  - that the expectation at a robust hit does not depend on the libm: the jittered oracle (every sine moved by a seeded -2 .. +2 ulp) gives
    the plain oracle's sample;
  - that a missed decision would be seen: the oracle's sample at a robust hit is at least 0.02 away from what an interpolating reader gives.
"""
import functools

import numpy as np
import pytest

import __graft_entry__ as entry
from helpers import TOL_RMS
import lfo_delay_ref as ref

CASES = ref.CASES
IDS = [ref.case_id(c) for c in CASES]
JITTER_SEEDS = (1, 2, 7)
FULL_RESTATEMENT_SAMPLES = 1100000


@functools.lru_cache(maxsize=None)
def case_inputs(k):
    x = ref.block_inputs(ref.case_seed(CASES[k]), CASES[k].frames)
    x.setflags(write=False)
    return x


def oracle_blocks(orc, unit, params, sr, x, calls):
    """[calls][frames]: the oracle's unit from zero state, call b fed x[b % len(x)]"""
    ch = orc.Chain()
    ch.append_unit(unit, params=params)
    out = np.empty((calls, x.shape[1]))
    for b in range(calls):
        out[b] = ch.process(x[b % len(x)], sr)
    del ch
    return out


@functools.lru_cache(maxsize=None)
def oracle_stream(k):
    """the plain oracle's stream of case k: computed once, never changed"""
    c = CASES[k]
    orc = entry.load_oracle()
    orc.build()
    out = oracle_blocks(orc, c.unit, c.params, c.sr, case_inputs(k), c.calls)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _hits(unit, params, sr, frames, calls):
    return tuple(ref.hits(unit, list(params), sr, frames, calls))


def case_hits(k):
    """the finder's hits of case k (the phaser's delay is the flanger's, expression for expression: phaser.go:64-71, flanger.go:58-65)"""
    c = CASES[k]
    return _hits("flanger" if c.unit == "phaser" else c.unit, tuple(c.params[:2]), c.sr, c.frames, c.calls)


def counted(k):
    """the hits the per-case counts are about: all but sample 0 of call 0 (sin(0) = 0 in every libm and every kernel)"""
    return [h for h in case_hits(k) if (h.call, h.sample) != (0, 0)]


def restated_call(k, call, **kw):
    """the restatement's block of one call of case k (the calls in front leave their state only)"""
    c = CASES[k]
    return ref.stream(c.unit, c.params, c.sr, c.frames, case_inputs(k).tolist(), call + 1, first=call, **kw)[0]


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_restatement_matches_the_oracle_bit_for_bit(k):
    c = CASES[k]
    first = 0 if c.frames * c.calls <= FULL_RESTATEMENT_SAMPLES else max(0, min(e[0] for e in c.expect) - 2)
    got = np.array(ref.stream(c.unit, c.params, c.sr, c.frames, case_inputs(k).tolist(), c.calls, first=first))
    want = oracle_stream(k)[first:]
    print("%s: calls %d .. %d restated, largest difference %.3e" % (IDS[k], first, c.calls - 1, float(np.abs(got - want).max())))
    assert np.array_equal(got, want), float(np.abs(got - want).max())


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_finder_returns_the_tables_hits(k):
    found = {(h.call, h.sample, h.lfo): h for h in case_hits(k)}
    for call, sample, lfo, delay, fragile in CASES[k].expect:
        assert (call, sample, lfo) in found, (call, sample, lfo)
        h = found[(call, sample, lfo)]
        assert (h.delay, not h.robust) == (delay, fragile), h
    for h in found.values():                        # what a whole delay means in the stream: the oracle reads the sample twice there
        assert 0 <= h.delay <= ref._Setup(CASES[k].unit, CASES[k].params, CASES[k].sr).size, h


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_every_case_holds_robust_sensitive_hits_and_few_fragile_ones(k):
    hs = counted(k)
    good = [h for h in hs if h.robust and h.sensitive]
    fragile = [h for h in hs if not h.robust]
    print("%s: %d hits, %d robust and sensitive, %d fragile" % (IDS[k], len(hs), len(good), len(fragile)))
    assert len(good) >= 2
    assert 2 * len(fragile) <= len(hs)


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_robust_hits_do_not_depend_on_the_libm(k):
    c = CASES[k]
    orc = entry.load_oracle()
    plain = oracle_stream(k)
    for seed in JITTER_SEEDS:
        with orc.jittered(seed):
            moved = oracle_blocks(orc, c.unit, c.params, c.sr, case_inputs(k), c.calls)
        for h in case_hits(k):
            if h.robust:
                assert abs(moved[h.call, h.sample] - plain[h.call, h.sample]) <= TOL_RMS, (seed, h)


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_a_missed_decision_at_a_robust_hit_would_be_seen(k):
    by_call = {}
    for h in counted(k):                            # (sample 0 of call 0 reads the empty delay buffer: twice nothing is nothing)
        if h.robust:
            by_call.setdefault(h.call, []).append(h)
    plain = oracle_stream(k)
    smallest = np.inf
    for call, hs in by_call.items():
        alt = restated_call(k, call, missed={(h.call, h.sample, h.lfo) for h in hs})
        for h in hs:
            smallest = min(smallest, abs(alt[h.sample] - plain[call, h.sample]))
    print("%s: a missed decision moves the sample by at least %.4f" % (IDS[k], smallest))
    assert smallest >= 0.02


def fragile_alternatives(k, h):
    """the restatement's sample at fragile hit h for each ulp offset -2 .. +2 of its sine"""
    return [restated_call(k, h.call, offsets={(h.call, h.sample, h.lfo): o})[h.sample] for o in ref.ULP_OFFSETS]


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_fragile_hits_have_two_answers_and_the_oracle_gives_one_of_them(k):
    fr = [h for h in case_hits(k) if not h.robust]
    plain = oracle_stream(k)
    for h in fr[:3]:
        alts = fragile_alternatives(k, h)
        assert plain[h.call, h.sample] == alts[ref.ULP_OFFSETS.index(0)]
        assert max(alts) - min(alts) >= 0.02, (h, alts)         # "whole" and "not whole" both occur within +-2 ulp: that is what fragile means
