"""Engine::BatchStreamOpen / Need / Step / Close of the C++ twin (host/gdg_host.hpp): one sliced job on a one-shard engine has the bytes
of Engine::BatchRun; an engine of several shards says that the streamed run is unsupported there."""
import numpy as np
import pytest

import __graft_entry__ as entry
from helpers import synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192


@pytest.fixture(scope="module")
def host():
    pkg = entry.load_package()
    pkg.build()
    from go_dsp_guitar_amd import host as h
    h.build()
    return h


def _engine(host, nch, sr, devices=None):
    irs = host.ImpulseResponses()
    irs.add("Cab", sr, -20, synth_ir(2000, seed=3))
    eng = host.Engine(nch, BLOCK, devices=devices)
    for c in range(nch):
        ch = eng.create_chain(irs)
        for t in (5, 19, 11):                                  # compressor, power amp, tone stack
            ch.SetBypass(ch.AppendUnit(t), False)
        ch.SetDiscreteValue(1, "filter_1", "Cab")
        ch.SetNumericValue(2, "middle", -3 - c)
    sp = host.Spatializer(eng, nch)
    sp.SetSampleRate(sr)
    for c in range(nch):
        sp.SetAzimuth(c, -50.0 + 30.0 * c); sp.SetDistance(c, 1.0 + 0.5 * c); sp.SetLevel(c, 0.9)
    m0 = eng.raw_context(0)
    m0.metronome_set_sounds(np.linspace(-0.5, 0.5, 700), np.linspace(0.4, -0.4, 400))
    m0.metronome_configure(3, 180, sr)
    return eng, sp


def _files(oracle, sr):
    lengths, rates = [30000, 70000, 0, 41000], [sr, 44100, sr, 96000]
    inputs = []
    for c, (n, rate) in enumerate(zip(lengths, rates)):
        inputs.append(None if n == 0 else (oracle.wave_encode("lpcm16", 0.7 * synth_signal(c, n, rate)), "lpcm16", rate))
    return inputs


def test_engine_streamed_job_has_the_bytes_of_batch_run(host, oracle):
    sr, nch = 48000, 4
    inputs = _files(oracle, sr)
    eng, sp = _engine(host, nch, sr)
    want = eng.batch_run(inputs, sr, "lpcm24", window=4, metronome_to_master=True)
    assert eng.last_error() == ""
    del sp
    eng.close()
    eng, sp = _engine(host, nch, sr)
    parts = list(eng.batch_stream(inputs, sr, "lpcm24", 3, window=4, metronome_to_master=True))
    assert eng.last_error() == ""
    assert len(parts) >= 3 and sum(p[0].size for p in parts) == want[0].size
    for r in range(nch + 3):
        np.testing.assert_array_equal(np.concatenate([p[r] for p in parts]), want[r], err_msg="output %d" % r)
    del sp
    eng.close()


def test_engine_of_several_shards_says_unsupported(host, oracle):
    sr, nch = 48000, 4
    eng, sp = _engine(host, nch, sr, devices=[0, 0])
    with pytest.raises(host.HostError, match="unsupported"):
        next(eng.batch_stream(_files(oracle, sr), sr, "lpcm24", 2))
    del sp
    eng.close()
