"""The Gram list through the C++ twin (Engine::SetBatchGram / LastBatchGram, host.py's gram= and render_matched): six channels render one
take through six different power amps, a seventh channel carries the target -- the IEEE64 render of 0.5 x1 + 0.25 x4, passed through an
empty chain -- and render_matched with up to three terms picks rigs 1 and 4, finds {0.5, 0.25} and stops.  gram= keeps the same records
through batch_run and through the streamed job, and a candidate given with a sign is measured as the port of a one-term blend."""
import numpy as np
import pytest

import __graft_entry__ as entry
from helpers import synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
SR, NCH, BLOCKS = 48000, 7, 3
NO = NCH + 3
EPS = 2.0 ** -52
NAMES = ("One", "Two", "Three", "Four", "Five", "Six")


@pytest.fixture(scope="module")
def host():
    entry.load_package()                                                 # build() has made both libraries
    from go_dsp_guitar_amd import host as h
    return h


def _engine(host):
    """six chains of one power amp each, with responses of different lengths, and an empty seventh chain"""
    irs = host.ImpulseResponses()
    for c, name in enumerate(NAMES):
        irs.add(name, SR, -20, synth_ir(1200 + 150 * c, seed=170 + c))
    eng = host.Engine(NCH, BLOCK)
    for name in NAMES:
        ch = eng.create_chain(irs)
        ch.SetBypass(ch.AppendUnit(19), False)                            # the power amp alone: the chain is linear
        ch.SetDiscreteValue(0, "filter_1", name)
    eng.create_chain(irs)                                                 # no unit: what comes in goes out
    sp = host.Spatializer(eng, NCH)
    sp.SetSampleRate(SR)
    for c in range(NCH):
        sp.SetAzimuth(c, -45.0 + 15.0 * c); sp.SetDistance(c, 1.0); sp.SetLevel(c, 0.9)
    eng.batch_set_sources([0] * 6 + [6])                                  # one take through six rigs; the target has its own file
    return eng, sp


def _take():
    """a take with a broad spectrum: the six renders span six dimensions"""
    x = 0.2 * synth_signal(0, BLOCKS * BLOCK - 300, SR) + 0.2 * np.random.default_rng(5).uniform(-1.0, 1.0, BLOCKS * BLOCK - 300)
    return (np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8), "lpcm16", SR)


LIST = [6, 0, 1, 2, 3, 4, 5]


@pytest.fixture(scope="module")
def renders(host):
    """the six renders of the take, and the Gram records of the list over that job"""
    eng, sp = _engine(host)
    outs = eng.batch_run([_take()] + [None] * 6, SR, "ieee64", window=2, gram=LIST)
    rows = [o.view(np.float64).copy() for o in outs]
    gram = eng.last_gram.copy()
    assert eng.last_error() == "" and len(rows) == NO and all(r.size == BLOCKS * BLOCK and np.isfinite(r).all() and r.any() for r in rows[:6]) and not rows[6].any()
    del sp
    eng.close()
    return rows, gram


def test_render_matched_picks_the_two_rigs_of_a_known_mix_and_stops(host, renders):
    rows, _ = renders
    mix = 0.5 * rows[1] + 0.25 * rows[4]
    inputs = [_take()] + [None] * 5 + [(np.ascontiguousarray(mix).view(np.uint8), "ieee64", SR)]
    eng, sp = _engine(host)
    outs, picked, weights, residuals = eng.render_matched(6, [0, 1, 2, 3, 4, 5], 3, inputs, SR, "ieee64", min_gain=1e-9, window=2)
    assert eng.last_error() == "" and len(outs) == NO + 1
    print("picked %r, weights %r, residuals %r" % (picked, weights, residuals))
    assert picked == [1, 4] and len(weights) == 2 and len(residuals) == 2      # the third candidate gains less than min_gain: it stops
    got = np.stack([o.view(np.float64) for o in outs])
    for c in range(6):                                                     # pass 2 starts from the saved state: the renders are those of a fresh engine
        assert np.array_equal(got[c], rows[c]), c
    # against numpy.linalg.lstsq on the downloaded float64 rows: the Gram's entries carry L * 2^-52 relative to sum |a b|, the solve
    # multiplies that by cond(G)
    X = got[[1, 4]]
    G = X @ X.T
    L = got.shape[1]
    tol = np.linalg.cond(G) * L * EPS
    want = np.linalg.lstsq(X.T, got[6], rcond=None)[0]
    print("cond %.3g, tolerance %.3g, weights off by %.3g" % (np.linalg.cond(G), tol, np.abs(np.array(weights) - want).max()))
    assert np.abs(np.array(weights) - want).max() <= tol, (weights, want, tol)
    assert np.abs(want - [0.5, 0.25]).max() <= 1e-6                        # ... which is the mix: the empty chain passes the target through
    # the rendered blend port against the target row: the planner's residual
    left = got[6] - got[NO]
    share = float(left @ left) / float(got[6] @ got[6])
    print("share left %.3g, the planner's %.3g" % (share, residuals[-1]))
    assert abs(share - residuals[-1]) <= tol, (share, residuals[-1], tol)
    assert residuals[0] > residuals[1] >= 0.0 and residuals[0] < 1.0
    assert eng.matched_records.shape == (BLOCKS, 7 * 8 // 2)
    del sp
    eng.close()


def test_gram_reaches_the_library_through_batch_run_and_the_streamed_job(host, renders):
    rows, gram = renders
    pkg = entry.load_package()
    assert gram.shape == (BLOCKS, 7 * 8 // 2)
    for b in range(BLOCKS):                                                # against the call's own files, to the bound of the definition
        s = slice(b * BLOCK, (b + 1) * BLOCK)
        for (i, j) in ((2, 1), (5, 5), (6, 3)):
            a, c = rows[LIST[i]][s], rows[LIST[j]][s]
            assert abs(gram[b, pkg.gram_index(i, j)] - a @ c) <= 2 * BLOCK * EPS * (np.abs(a) @ np.abs(c)), (b, i, j)      # numpy's own sum carries as much again
        assert not gram[b, :1].any()                                       # the seventh channel had no file: a silent row
    eng, sp = _engine(host)
    parts = list(eng.batch_stream([_take()] + [None] * 6, SR, "ieee64", 2, window=2, gram=LIST))
    assert len(parts) == 2 and eng.last_gram.tobytes() == gram.tobytes()
    with pytest.raises(host.HostError, match="list entry 2 names port 1, which entry 0 names already"):
        eng._set_gram([1, 2, 1])
    assert host.lib().gdgh_engine_batch_gram_ports(eng._h) == 7           # a refused list leaves the one in force
    with pytest.raises(host.HostError, match="list entry 1 names port %d" % NO):
        eng.batch_run([_take()] + [None] * 6, SR, "ieee64", window=2, gram=[0, NO])
    assert eng._set_gram(None) == 0
    del sp
    eng.close()


def test_a_candidate_with_a_sign_is_measured_as_a_one_term_blend(host, renders):
    """the target is channel 0; the candidates are channel 0 with its polarity turned and channel 2: the list holds the port of the blend
    -1 * x0, the planner picks it with the weight -1, and pass 2 writes sign * weight = +1: the blend port is channel 0's file"""
    rows, _ = renders
    eng, sp = _engine(host)
    outs, picked, weights, residuals = eng.render_matched(0, [(0, 0, -1), 2], 2, [_take()] + [None] * 6, SR, "ieee64", min_gain=1e-9, window=2)
    assert picked == [0] and abs(weights[0] + 1.0) <= 1e-12 and residuals[0] <= 1e-12
    got = [o.view(np.float64) for o in outs]
    assert len(got) == NO + 1 and np.array_equal(got[0], rows[0]) and np.abs(got[NO] - rows[0]).max() <= 1e-12 * np.abs(rows[0]).max()
    del sp
    eng.close()
