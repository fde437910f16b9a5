"""The records of the delivered rows through the C++ twin (Engine::SetBatchDelivered / LastBatchDelivered, host.py's delivered=True): the
engine's records are the library's stand-alone call on the engine's own float64 files, whole and streamed (the pieces concatenated along
blocks), and an engine of more shards refuses the switch."""
import numpy as np
import pytest

import __graft_entry__ as entry
import delivered_ref as ref

pytestmark = pytest.mark.gpu

BLOCK = 8192
SR = 96000


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


def test_the_engine_s_records_are_the_library_s_of_its_files(host):
    pkg = entry.load_package()
    triple = (2, 147, 160)
    n = 3 * BLOCK
    x = 0.9 * np.sign(np.sin(2.0 * np.pi * 1000.0 * np.arange(n) / SR)) + 0.1 * np.random.default_rng(3).uniform(-1, 1, n)
    inputs = [(np.ascontiguousarray(x).view(np.uint8), "ieee64", SR)]
    ctx = pkg.Context(1, BLOCK)
    for deliver in (None, triple):
        eng, sp = _engine(host)                                          # a fresh engine per job: everything starts from rest
        outs = eng.batch_run(inputs, SR, "ieee64", window=2, deliver=deliver, delivered=True)
        whole = eng.last_delivered
        assert eng.last_error() == "" and whole.shape == (4, 3) and whole.dtype == pkg.BLOCK_DELIVERED_DTYPE
        del sp
        eng.close()
        span = ref.spans(*(deliver or (1, 1, 1)), 0, 3, pkg.batch_delivery_samples)
        want = ctx.block_delivered_rows(np.stack([o.view(np.float64) for o in outs]), span)
        assert whole.tobytes() == want.tobytes(), deliver
        assert whole["true_peak"][0].max() > whole["peak"][0].max()
        eng, sp = _engine(host)
        for _ in eng.batch_stream(inputs, SR, "ieee64", lambda left: 1 if left == 3 else 2, window=2, deliver=deliver, delivered=True):
            pass
        assert eng.last_delivered.shape == (4, 3) and eng.last_delivered.tobytes() == want.tobytes(), deliver
        outs = eng.batch_run(inputs, SR, "ieee64", window=2, deliver=deliver)      # the default: none are kept
        assert eng.last_delivered is None
        del sp
        eng.close()
    ctx.close()


def test_an_engine_of_more_shards_refuses_the_switch(host):
    data = [(np.zeros(8 * BLOCK, dtype=np.uint8), "ieee64", SR)]
    eng, sp = _engine(host, devices=[0, 0], nch=2)
    assert eng.shards() == 2
    with pytest.raises(host.HostError, match="SetBatchDelivered: the engine has 2 shards.*gdg_batch_out_records_enable"):
        eng.batch_run(data * 2, SR, "ieee64", delivered=True)
    with pytest.raises(host.HostError, match="SetBatchDelivered"):
        eng.render_normalized(-1.0, 40.0, data * 2, SR, "ieee64", measure="delivered")
    outs = eng.batch_run(data * 2, SR, "ieee64", window=1)               # usable afterwards
    assert outs[0].size == 8 * BLOCK
    del sp
    eng.close()
    with pytest.raises(ValueError):
        eng.render_normalized(-1.0, 40.0, data * 2, SR, "ieee64", measure="files")
