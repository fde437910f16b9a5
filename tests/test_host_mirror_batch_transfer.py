"""The transfer records through the C++ twin (Engine::SetBatchTransfers / LastBatchTransfer, host.py's transfers= and match_ir): white noise
shared by two channels, channel 0 through a unit impulse, channel 1 through a power amp with a random 12-tap response.  The records the
engine keeps are the bytes Context.block_transfer gives for the call's own float64 files -- which tests/test_gpu_transfer.py holds equal to
Context.batch_transfer -- whether the job runs in one call or in slices; and match_ir leaves the engine as it found it: a render after it is
byte for byte the render of an engine that never ran it."""
import numpy as np
import pytest

import transfer_ref as ref
import __graft_entry__ as entry

BLOCK = 8192
SR, NCH, BLOCKS = 48000, 2, 3
NO = NCH + 3
SAMPLES = BLOCKS * BLOCK - 300
IR_TAPS = 12
GROUP = 32
PAIRS = [(0, 1), (1, NCH)]


def take(seed=1):
    x = np.random.default_rng(seed).standard_normal(SAMPLES)
    return np.round(0.25 * x / 4.0 * 32767.0).clip(-32767, 32767) / 32767.0


def amp_ir(seed=1):
    return np.random.default_rng(100 + seed).uniform(-1.0, 1.0, IR_TAPS)


@pytest.fixture(scope="module")
def host():
    entry.load_package()                                                 # build() has made both libraries
    from go_dsp_guitar_amd import host as h
    return h


def _engine(host):
    irs = host.ImpulseResponses()
    unit = np.zeros(IR_TAPS)
    unit[0] = 1.0
    irs.add("Wire", SR, -20, unit)
    irs.add("Amp", SR, -20, amp_ir())
    eng = host.Engine(NCH, BLOCK)
    for name in ("Wire", "Amp"):
        ch = eng.create_chain(irs)
        ch.SetBypass(ch.AppendUnit(19), False)                            # the power amp alone: the chain is linear
        ch.SetDiscreteValue(0, "filter_1", name)
    sp = host.Spatializer(eng, NCH)
    sp.SetSampleRate(SR)
    for c in range(NCH):
        sp.SetAzimuth(c, -30.0 + 60.0 * c); sp.SetDistance(c, 1.0); sp.SetLevel(c, 0.9)
    eng.batch_set_sources([0, 0])                                         # one take through two rigs
    return eng, sp


def _inputs():
    return [(np.ascontiguousarray(np.round(take() * 32767.0).astype("<i2")).view(np.uint8), "lpcm16", SR), None]


def test_every_layer_of_the_twin_knows_the_calls(host):
    import os
    assert callable(host.Engine._set_transfers) and callable(host.Engine.match_ir)
    for name in ("gdgh_engine_set_batch_transfers", "gdgh_engine_batch_transfers", "gdgh_engine_last_batch_transfer"):
        assert getattr(host.lib(), name) is not None
    with open(os.path.join(entry.PKG_DIR, "host", "gdg_host.hpp")) as f:
        hpp = f.read()
    assert "Error SetBatchTransfers(const std::vector<TransferPair> &pairs, int group);" in hpp
    assert "Error LastBatchTransfer(std::vector<double> &records, size_t *blocks, size_t *doublesPerBlock) const;" in hpp


@pytest.mark.gpu
def test_last_batch_transfer_is_the_context_s_record_of_the_call_s_own_files(host):
    pkg = entry.load_package()
    eng, sp = _engine(host)
    outs = eng.batch_run(_inputs(), SR, "ieee64", window=2, transfers=(PAIRS, GROUP))
    assert eng.last_error() == "" and len(outs) == NO
    rows = np.stack([o.view(np.float64) for o in outs])
    assert eng.last_transfer.shape == (BLOCKS, ref.doubles(len(PAIRS), GROUP)) and eng.last_transfer.any()
    ctx = pkg.Context(1, BLOCK)
    want = ctx.block_transfer(rows, PAIRS, GROUP).reshape(BLOCKS, -1)
    assert eng.last_transfer.tobytes() == want.tobytes()
    # in slices: the engine goes on from where the first job left its chains, so the rows are this job's own
    parts = list(eng.batch_stream(_inputs(), SR, "ieee64", 2, window=2, transfers=(PAIRS, GROUP)))
    rows = np.stack([np.concatenate([part[r].view(np.float64) for part in parts]) for r in range(NO)])
    want = ctx.block_transfer(rows, PAIRS, GROUP).reshape(BLOCKS, -1)
    ctx.close()
    assert len(parts) == 2 and eng.last_transfer.shape == want.shape and eng.last_transfer.tobytes() == want.tobytes()
    # refusals name the pair and leave the list in force
    assert eng._set_transfers((PAIRS, GROUP)) == 2
    for transfers, what in (((PAIRS, 3), "a group width of 3 bins"), (([(0, -1)], 1), "pair 0 has the target port -1"), (([(0, 1)] * 17, 1), "17 pairs")):
        with pytest.raises(host.HostError, match=what):
            eng._set_transfers(transfers)
        assert host.lib().gdgh_engine_batch_transfers(eng._h) == 2
    eng.batch_run(_inputs(), SR, "ieee64", window=2, skip_outputs=True)       # off again: the call keeps none
    assert eng.last_transfer is None and host.lib().gdgh_engine_batch_transfers(eng._h) == 0
    del sp
    eng.close()


@pytest.mark.gpu
def test_match_ir_returns_the_planner_s_taps_and_leaves_the_engine_as_it_found_it(host):
    pkg = entry.load_package()
    eng, sp = _engine(host)
    taps, coherence = eng.match_ir(0, 1, 16, _inputs(), SR, "ieee64", group=GROUP, center=0, window=2)
    assert taps.shape == (16,) and 0.9 < coherence <= 1.0 + 1e-9 and eng.match_records.shape == (BLOCKS, ref.doubles(1, GROUP))
    want, want_coh = pkg.match_taps_from_transfer(eng.match_records, 1, GROUP, 16, 0)
    assert taps.tobytes() == want[0].tobytes() and coherence == want_coh[0]
    assert host.lib().gdgh_engine_batch_transfers(eng._h) == 0
    after = eng.batch_run(_inputs(), SR, "ieee64", window=2)
    del sp
    eng.close()
    fresh, sp = _engine(host)
    never = fresh.batch_run(_inputs(), SR, "ieee64", window=2)
    del sp
    fresh.close()
    assert len(after) == len(never) == NO
    for r in range(NO):
        assert np.array_equal(after[r], never[r]), r
