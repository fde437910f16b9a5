"""The delivery through the C++ twin (Engine::SetBatchDelivery, host.py's deliver= argument): a 440 Hz and a 30 kHz sine summed at 96 kHz and
delivered at factor 2.  The 440 Hz line comes out at A times the anti-aliasing filter's gain there, and the 30 kHz line -- which a bare
decimation would fold to 18 kHz at full level -- lies at the filter's stop-band level at 30 kHz; both figures are computed from the taps
(tests/deliver_ref.py restates them from csrc/aa_taps.h), none is assumed.  And what the twin refuses."""
import numpy as np
import pytest

import deliver_ref as ref
import __graft_entry__ as entry

pytestmark = pytest.mark.gpu

BLOCK = 8192
SR, F_LOW, F_HIGH, AMP = 96000, 440.0, 30000.0, 0.3


@pytest.fixture(scope="module")
def host():
    entry.load_package()                                                 # build() has made both libraries
    from go_dsp_guitar_amd import host as h
    return h


def _engine(host, devices=None, nch=1):
    eng = host.Engine(nch, BLOCK, devices=devices)
    irs = host.ImpulseResponses()
    for _ in range(nch):
        ch = eng.create_chain(irs)
        ch.AppendUnit(11)                                                # a tone stack, left bypassed: the chain hands its input on
    sp = host.Spatializer(eng, nch)
    sp.SetSampleRate(SR)
    return eng, sp


def _lines(y, rate, freqs, skip):
    """amplitudes of the sines at `freqs` in y[skip:], by least squares on their sines and cosines"""
    t = np.arange(skip, y.size) / float(rate)
    basis = np.stack([f(2.0 * np.pi * fr * t) for fr in freqs for f in (np.sin, np.cos)], axis=1)
    coef, *_ = np.linalg.lstsq(basis, y[skip:], rcond=None)
    return [float(np.hypot(coef[2 * i], coef[2 * i + 1])) for i in range(len(freqs))]


def _gain(h, freq, rate):
    """|H(e^{j w})| of the taps at `freq`"""
    w = 2.0 * np.pi * freq / rate
    return float(abs(np.sum(h * np.exp(-1j * w * np.arange(h.size)))))


def test_the_passband_line_and_the_aliased_line(host):
    n = 2 * BLOCK
    t = np.arange(n) / float(SR)
    x = AMP * np.sin(2.0 * np.pi * F_LOW * t) + AMP * np.sin(2.0 * np.pi * F_HIGH * t)
    inputs = [(np.ascontiguousarray(x).view(np.uint8), "ieee64", SR)]
    outs = {}
    for deliver in (None, 2):
        eng, sp = _engine(host)                                          # a fresh engine per job: everything starts from rest
        outs[deliver] = eng.batch_run(inputs, SR, "ieee64", window=2, deliver=deliver)[0].view(np.float64).copy()
        assert eng.last_error() == ""
        del sp
        eng.close()
    assert outs[None].size == n and outs[2].size == n // 2
    h = ref.taps(2)
    # what the chain hands to the delivery: the two lines of the session-rate row
    low_in, high_in = _lines(outs[None], SR, (F_LOW, F_HIGH), 0)
    assert abs(low_in - AMP) < 1e-6 and abs(high_in - AMP) < 1e-6     # a bypassed chain hands its input on
    # the delivered row at 48 kHz, behind the filter's 76 session samples of start-up: 440 Hz, and 18 kHz where 30 kHz folds to
    low, folded = _lines(outs[2], SR // 2, (F_LOW, SR / 2.0 - F_HIGH), ref.TAPS[2])
    pass_gain, stop_gain = _gain(h, F_LOW, SR), _gain(h, F_HIGH, SR)
    print("passband gain at 440 Hz %.9f, stop-band gain at 30 kHz %.3e (%.1f dB); lines %.9f and %.3e" % (pass_gain, stop_gain, 20 * np.log10(stop_gain), low, folded))
    assert 0.94 < pass_gain < 1.06 and stop_gain < 1e-5                     # +-0.5 dB, and 100 dB at least: the table's own figures, printed above
    assert abs(low - ref.A * pass_gain * low_in) <= 1e-9 * low_in
    # below the stop-band level of the same taps at 30 kHz (the fit's own rounding, 1e-12, on top)
    assert folded <= ref.A * stop_gain * high_in * (1.0 + 1e-6) + 1e-12
    assert folded < 1e-5 * high_in                                         # ... which is nothing like the full-level line a bare decimation leaves


def test_the_twin_refuses_what_the_library_would(host):
    eng, sp = _engine(host)
    with pytest.raises(host.HostError, match="delivery factor 3"):
        eng.batch_run([(np.zeros(8 * BLOCK, dtype=np.uint8), "ieee64", SR)], SR, "ieee64", deliver=3)
    del sp
    eng.close()
    eng, sp = _engine(host, devices=[0, 0], nch=2)
    assert eng.shards() == 2
    with pytest.raises(host.HostError, match="2 shards.*delivery factor 2 needs a one-shard engine"):
        eng.batch_run([(np.zeros(8 * BLOCK, dtype=np.uint8), "ieee64", SR)] * 2, SR, "ieee64", deliver=2)
    outs = eng.batch_run([(np.zeros(8 * BLOCK, dtype=np.uint8), "ieee64", SR)] * 2, SR, "ieee64", window=1)      # usable afterwards, at the session rate
    assert outs[0].size == 8 * BLOCK
    del sp
    eng.close()
