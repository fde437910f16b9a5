"""All nine record kinds of the C++ twin at once (host/batch_records.h under Engine::LastBatch*, host.py's one record table): a table
loop can file one kind into another's store, and no other test turns on more than two kinds together.  One short job -- two channels,
compressor and tone stack, 48 kHz, three blocks -- with every kind and one blend on: every last_* of that one call is, bit for bit, the
last_* of a call with only that kind (and the blend) on, the streamed job's are batch_run's, and an engine of two shards files the four
port kinds where the one-shard engine does."""
import numpy as np
import pytest

import __graft_entry__ as entry
import spectrum_ref
from test_gpu_block_stats import check_records, ref_stats

pytestmark = pytest.mark.gpu

BLOCK = 8192
SR, NCH, BLOCKS = 48000, 2, 3
N3 = NCH + 3
BLENDS = [[(0, 0.5), (1, -0.25)]]                                        # port N3
KINDS = {                                                                # the batch calls' argument that turns a kind on, by its last_* name
    "last_report": dict(report=True),
    "last_spectrum": dict(spectrum=[0.0, 200.0, 2000.0, 20000.0]),
    "last_align": dict(align=([0, 0, 0, -1, N3 - 1, 1], 64)),            # the master and the blend port are measured too
    "last_true_peak": dict(true_peak=True),
    "last_fit": dict(fits=[(0, [1, N3])]),
    "last_gram": dict(gram=[0, 1, N3]),
    "last_tapfit": dict(tapfits=[(0, [1], 4)]),
    "last_transfer": dict(transfers=([(1, 0)], 32)),
    "last_delivered": dict(delivered=True),
}
PORT_KINDS = ("last_report", "last_spectrum", "last_align", "last_true_peak")
ALL = {k: v for kw in KINDS.values() for k, v in kw.items()}


@pytest.fixture(scope="module")
def host():
    entry.load_package()                                                 # build() has made both libraries
    from go_dsp_guitar_amd import host as h
    return h


def _inputs():
    rng = np.random.default_rng(11)
    t = np.arange(BLOCKS * BLOCK)
    return [(np.ascontiguousarray(0.4 * np.sin(2.0 * np.pi * 220.0 * (c + 1) * t / SR) + 0.1 * rng.uniform(-1, 1, t.size)).view(np.uint8), "ieee64", SR)
            for c in range(NCH)]


def _run(host, devices=None, slices=None, **kw):
    """a fresh engine (everything starts from rest), one job: (outs, {last_* name: records or None})"""
    eng = host.Engine(NCH, BLOCK, devices=devices)
    irs = host.ImpulseResponses()
    for c in range(NCH):
        ch = eng.create_chain(irs)
        for t in (5, 11):                                                # compressor, tone stack: a short chain without a power amp
            ch.SetBypass(ch.AppendUnit(t), False)
        ch.SetNumericValue(1, "middle", -3 - c)
    sp = host.Spatializer(eng, NCH)
    sp.SetSampleRate(SR)
    for c in range(NCH):
        sp.SetAzimuth(c, -40.0 + 80.0 * c); sp.SetDistance(c, 1.0 + 0.5 * c); sp.SetLevel(c, 0.9)
    m0 = eng.raw_context(0)
    m0.metronome_set_sounds(np.linspace(-0.5, 0.5, 700), np.linspace(0.4, -0.4, 400))
    m0.metronome_configure(3, 180, SR)
    if slices is None:
        outs = eng.batch_run(_inputs(), SR, "ieee64", window=2, metronome_to_master=True, **kw)
    else:
        it = iter(slices)
        parts = list(eng.batch_stream(_inputs(), SR, "ieee64", lambda left: next(it), window=2, metronome_to_master=True, **kw))
        assert len(parts) == len(slices)
        outs = [np.concatenate([p[r] for p in parts]) for r in range(len(parts[0]))]
    assert eng.last_error() == ""
    last = {name: getattr(eng, name) for name in KINDS}
    del sp
    eng.close()
    return outs, last


@pytest.fixture(scope="module")
def everything(host):
    return _run(host, blends=BLENDS, **ALL)


def test_every_kind_beside_the_eight_others_is_the_kind_alone(host, everything):
    pkg = entry.load_package()
    outs, last = everything
    assert len(outs) == N3 + 1 and all(o.size == BLOCKS * BLOCK * 8 for o in outs)
    shapes = {"last_report": (N3 + 1, BLOCKS), "last_spectrum": (N3 + 1, BLOCKS, 3), "last_align": (N3 + 1, BLOCKS), "last_true_peak": (N3 + 1, BLOCKS),
              "last_fit": (1, BLOCKS), "last_gram": (BLOCKS, 6), "last_tapfit": (BLOCKS, last["last_tapfit"].shape[1]),
              "last_transfer": (BLOCKS, (4096 // 32 + 1) * 4), "last_delivered": (N3 + 1, BLOCKS)}
    dtypes = {"last_report": pkg.BLOCK_STATS_DTYPE, "last_align": pkg.BLOCK_ALIGN_DTYPE, "last_true_peak": pkg.BLOCK_TRUE_PEAK_DTYPE, "last_fit": pkg.FIT_DTYPE,
              "last_delivered": pkg.BLOCK_DELIVERED_DTYPE}
    for name, kw in KINDS.items():
        assert last[name].shape == shapes[name] and last[name].dtype == dtypes.get(name, np.float64), name
        assert any(last[name].tobytes()), name + ": not all zero"
        alone_outs, alone = _run(host, blends=BLENDS, **kw)
        assert alone[name].shape == last[name].shape and alone[name].tobytes() == last[name].tobytes(), name
        assert [k for k in KINDS if alone[k] is not None] == [name], "the other kinds are off"
        assert [o.tobytes() for o in alone_outs] == [o.tobytes() for o in outs], name + ": the records change no output byte"


def test_the_streamed_job_keeps_batch_run_s_records_of_every_kind(host, everything):
    outs, last = everything
    for slices in ([1, 2], [2, 1]):
        got_outs, got = _run(host, slices=slices, blends=BLENDS, **ALL)
        for name in KINDS:
            assert got[name].shape == last[name].shape and got[name].tobytes() == last[name].tobytes(), (name, slices)
        assert [o.tobytes() for o in got_outs] == [o.tobytes() for o in outs], slices


def test_two_shards_file_the_four_port_kinds_where_one_shard_does(host):
    """Chain and metronome rows come from the shards and are the one-shard engine's on the bytes.  The master rows come from the finish,
    which adds two partial mixes where the one-shard engine has one, so its sums are associated differently: they are held to the
    bounds of the per-kind tests -- the true peak within 1e-12 relative (test_host_mirror_batch_true_peak.py), the bands within
    1e-12 * T, T = the numpy restatement's sum over all bins of the block (test_host_mirror_batch_spectrum.py), and the report against
    numpy on the engine's own IEEE64 master files, exact fields exactly and sum_sq within n * 2^-52 (test_host_mirror_batch_report.py)."""
    on = {k: v for name in PORT_KINDS for k, v in KINDS[name].items()}
    on["align"] = ([0, 1, -1, -1, N3 - 1], 64)                          # every port against one on its own shard; no master port over shards
    one_outs, one = _run(host, **on)
    two_outs, two = _run(host, devices=[0, 0], **on)
    keep = list(range(NCH)) + [N3 - 1]                                   # chain outputs and the metronome; the finish makes the master
    master = [NCH, NCH + 1]
    for name in PORT_KINDS:
        assert two[name].shape == one[name].shape == (N3, BLOCKS) + one[name].shape[2:], name
        assert two[name][keep].tobytes() == one[name][keep].tobytes() and any(two[name][keep].tobytes()), name
    for name in set(KINDS) - set(PORT_KINDS):
        assert one[name] is None and two[name] is None, name
    edges = KINDS["last_spectrum"]["spectrum"]
    for what, outs, last in (("one shard", one_outs, one), ("two shards", two_outs, two)):
        rows = np.stack([o.view(np.float64) for o in outs])
        assert rows.shape == (N3, BLOCKS * BLOCK) and rows[master].any()
        assert last["last_align"][master].tobytes() == bytes(last["last_align"].dtype.itemsize * 2 * BLOCKS), what + ": the master rows are zero records"
        check_records(last["last_report"], np.stack([ref_stats(r, BLOCK) for r in rows]), BLOCK, what + ": the report, master rows included")
        for side in master:
            tp, tp_one = last["last_true_peak"][side]["true_peak"], one["last_true_peak"][side]["true_peak"]
            print("%s, master row %d: true peak %r (one shard %r)" % (what, side, tp, tp_one))
            assert np.all(tp_one > 0.0) and np.all(np.abs(tp - tp_one) <= 1e-12 * tp_one), (what, side)
            bands, total = spectrum_ref.block_spectrum(one_outs[side].view(np.float64), SR, edges)
            print("%s, master row %d: bands against the one-shard engine's, worst |d| / T %.3g" % (what, side, np.max(np.abs(last["last_spectrum"][side] - one["last_spectrum"][side]) / total[:, None])))
            assert np.all(total > 0.0) and last["last_spectrum"][side].any()
            assert np.all(np.abs(last["last_spectrum"][side] - one["last_spectrum"][side]) <= 1e-12 * total[:, None]), (what, side)
            assert np.all(np.abs(one["last_spectrum"][side] - bands) <= 1e-12 * total[:, None]), (what, side)      # ... which are the restatement's of its own master file
