"""The ratio stage through the C++ twin (Engine::SetBatchDelivery(factor, up, down), host.py's deliver=(factor, up, down) and delivery_for):
the engine's bytes are the library call's, whole and streamed, and the twin refuses what the library would."""
import numpy as np
import pytest

import deliver_ratio_ref as ref
import __graft_entry__ as entry

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


def test_the_engine_s_bytes_are_the_library_s(host):
    pkg = entry.load_package()
    triple = host.delivery_for(SR, 44100)
    assert triple == (2, 147, 160) == ref.rate_triple(SR, 44100)
    n = 3 * BLOCK
    x = 0.3 * np.sin(2.0 * np.pi * 440.0 * np.arange(n) / SR) + 0.1 * np.random.default_rng(3).uniform(-1, 1, n)
    inputs = [(np.ascontiguousarray(x).view(np.uint8), "ieee64", SR)]
    outs = {}
    for deliver in (None, triple):
        eng, sp = _engine(host)                                          # a fresh engine per job: everything starts from rest
        outs[deliver] = [o.view(np.float64).copy() for o in eng.batch_run(inputs, SR, "ieee64", window=2, deliver=deliver)]
        assert eng.last_error() == ""
        del sp
        eng.close()
    eng, sp = _engine(host)
    pieces = list(eng.batch_stream(inputs, SR, "ieee64", 1, window=2, deliver=triple))
    del sp
    eng.close()
    count = pkg.batch_delivery_samples(*triple, 0, n)
    assert count == ref.delivered_samples(*triple, 0, n)
    assert [p[0].size // 8 for p in pieces] == [pkg.batch_delivery_samples(*triple, b * BLOCK, BLOCK) for b in range(3)]
    ctx = pkg.Context(1, BLOCK)
    for r in range(4):
        row = outs[None][r]
        want = ctx.deliver_rows_ratio(ctx.deliver_rows(row, triple[0]), triple[1], triple[2])
        assert want.size == count and np.array_equal(outs[triple][r], want), r
        assert np.array_equal(np.concatenate([p[r] for p in pieces]).view(np.float64), want), r
    ctx.close()


def test_the_twin_refuses_what_the_library_would(host):
    eng, sp = _engine(host)
    data = [(np.zeros(8 * BLOCK, dtype=np.uint8), "ieee64", SR)]
    for bad, text in (((1, 294, 320), "delivery ratio 294/320"), ((1, 1, 3), "delivery ratio 1/3"), ((3, 147, 160), "delivery factor 3")):
        with pytest.raises(host.HostError, match=text):
            eng.batch_run(data, SR, "ieee64", deliver=bad)
    del sp
    eng.close()
    eng, sp = _engine(host, devices=[0, 0], nch=2)
    assert eng.shards() == 2
    with pytest.raises(host.HostError, match="2 shards.*delivery ratio 147/160 needs a one-shard engine"):
        eng.batch_run(data * 2, SR, "ieee64", deliver=(1, 147, 160))
    outs = eng.batch_run(data * 2, SR, "ieee64", window=1)               # usable afterwards, at the session rate
    assert outs[0].size == 8 * BLOCK
    del sp
    eng.close()
    with pytest.raises(ValueError):
        host.delivery_for(192000, 8000)
