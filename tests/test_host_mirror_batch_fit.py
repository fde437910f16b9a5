"""The blend fit through the C++ twin (Engine::SetBatchFits / LastBatchFit, host.py's fits= and render_fitted): three channels render one
take through three power amps, a fourth channel carries the target -- the IEEE64 render of 0.5 x0 + 0.25 x1, passed through an empty
chain -- and render_fitted finds {0.5, 0.25} again.  The file round trip is float64, so the 1e-6 is slack for the chain's pass-through
alone.  fits= keeps the same records through batch_run and through the streamed job, and a term given with a sign is fitted as the port
of a one-term blend."""
import numpy as np
import pytest

import __graft_entry__ as entry
from helpers import synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
SR, NCH, BLOCKS = 48000, 4, 3
NO = NCH + 3


@pytest.fixture(scope="module")
def host():
    entry.load_package()                                                 # build() has made both libraries
    from go_dsp_guitar_amd import host as h
    return h


def _engine(host):
    """three chains of one power amp each, with responses of one length and one energy, and an empty fourth chain"""
    irs = host.ImpulseResponses()
    for c, name in enumerate(("One", "Two", "Three")):
        irs.add(name, SR, -20, synth_ir(2000, seed=70 + c))
    eng = host.Engine(NCH, BLOCK)
    for name in ("One", "Two", "Three"):
        ch = eng.create_chain(irs)
        ch.SetBypass(ch.AppendUnit(19), False)                            # the power amp alone: the chain is linear
        ch.SetDiscreteValue(0, "filter_1", name)
    eng.create_chain(irs)                                                 # no unit: what comes in goes out
    sp = host.Spatializer(eng, NCH)
    sp.SetSampleRate(SR)
    for c in range(NCH):
        sp.SetAzimuth(c, -45.0 + 30.0 * c); sp.SetDistance(c, 1.0); sp.SetLevel(c, 0.9)
    eng.batch_set_sources([0, 0, 0, 3])                                   # one take through three rigs; the target has its own file
    return eng, sp


def _take():
    """a take with a broad spectrum: two sines alone would leave every render in one four-dimensional space"""
    x = 0.2 * synth_signal(0, BLOCKS * BLOCK - 300, SR) + 0.2 * np.random.default_rng(5).uniform(-1.0, 1.0, BLOCKS * BLOCK - 300)
    return (np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8), "lpcm16", SR)


@pytest.fixture(scope="module")
def renders(host):
    """the three renders of the take, and the fit records of (target 0; terms 1, 2) of that job"""
    eng, sp = _engine(host)
    outs = eng.batch_run([_take(), None, None, None], SR, "ieee64", window=2, fits=[(0, [1, 2])])
    rows = [o.view(np.float64).copy() for o in outs]
    fit = eng.last_fit.copy()
    assert eng.last_error() == "" and len(rows) == NO and all(r.size == BLOCKS * BLOCK and np.isfinite(r).all() and r.any() for r in rows[:3]) and not rows[3].any()
    del sp
    eng.close()
    return rows, fit


def test_render_fitted_finds_the_weights_of_a_known_mix(host, renders):
    rows, _ = renders
    G = np.array([[rows[j] @ rows[k] for k in range(2)] for j in range(2)])
    assert np.linalg.cond(G) <= 1e3, np.linalg.cond(G)                      # the two rigs differ enough
    mix = 0.5 * rows[0] + 0.25 * rows[1]
    inputs = [_take(), None, None, (np.ascontiguousarray(mix).view(np.uint8), "ieee64", SR)]
    eng, sp = _engine(host)
    outs, weights, residual = eng.render_fitted(3, [0, 1], inputs, SR, "ieee64", window=2)
    assert eng.last_error() == "" and len(outs) == NO + 1
    print("weights %r, residual %.3g" % (weights, residual))
    assert len(weights) == 2 and abs(weights[0] - 0.5) <= 1e-6 and abs(weights[1] - 0.25) <= 1e-6
    assert 0.0 <= residual <= 1e-10
    got = [o.view(np.float64) for o in outs]
    for c in range(3):                                                     # pass 2 starts from the saved state: the renders are those of a fresh engine
        assert np.array_equal(got[c], rows[c]), c
    assert np.abs(got[3] - mix).max() <= 1e-6 * np.abs(mix).max()          # the empty chain passes the target through
    assert np.abs(got[NO] - mix).max() <= 1e-5 * np.abs(mix).max()         # ... and the fitted blend is the mix again
    rec = eng.fitted_records
    assert rec.shape == (1, BLOCKS) and (rec["terms"] == 2).all() and not rec["skipped"].any()
    del sp
    eng.close()


def test_fits_reach_the_library_through_batch_run_and_the_streamed_job(host, renders):
    rows, fit = renders
    entry_pkg = entry.load_package()
    assert fit.shape == (1, BLOCKS) and fit.dtype == entry_pkg.FIT_DTYPE and (fit["terms"] == 2).all()
    for b in range(BLOCKS):                                                # against the call's own files, to the products' rounding
        s = slice(b * BLOCK, (b + 1) * BLOCK)
        assert abs(fit[0, b]["tx"][1] - rows[0][s] @ rows[2][s]) <= BLOCK * 2.0 ** -52 * (np.abs(rows[0][s]) @ np.abs(rows[2][s]))
    eng, sp = _engine(host)
    parts = list(eng.batch_stream([_take(), None, None, None], SR, "ieee64", 2, window=2, fits=[(0, [1, 2])]))
    assert len(parts) == 2 and eng.last_fit.tobytes() == fit.tobytes()
    with pytest.raises(host.HostError, match="fit 0 has 9 terms"):
        eng._set_fits([(0, [1] * 9)])
    assert host.lib().gdgh_engine_batch_fits(eng._h) == 1                 # a refused list leaves the one in force
    with pytest.raises(host.HostError, match="fit 0, term 0 names port %d" % NO):
        eng.batch_run([_take(), None, None, None], SR, "ieee64", window=2, fits=[(0, [NO])])
    assert eng._set_fits(None) == 0
    del sp
    eng.close()


def test_a_term_with_a_sign_is_fitted_as_a_one_term_blend(host, renders):
    """the target is channel 0 and the one term is channel 0 with its polarity turned: the fit sees the port of the blend -1 * x0, finds -1,
    and pass 2 writes sign * weight = +1: the blend port is channel 0's file"""
    rows, _ = renders
    eng, sp = _engine(host)
    outs, weights, residual = eng.render_fitted(0, [0], [_take(), None, None, None], SR, "ieee64", signs=[-1], delays=[0], window=2)
    assert abs(weights[0] + 1.0) <= 1e-12 and residual <= 1e-12
    got = [o.view(np.float64) for o in outs]
    assert len(got) == NO + 1 and np.array_equal(got[0], rows[0]) and np.abs(got[NO] - rows[0]).max() <= 1e-12 * np.abs(rows[0]).max()
    del sp
    eng.close()
