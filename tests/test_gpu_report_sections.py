"""The sections of the render report's four record kinds in a batch call's download half (csrc/report_sections.h) on the device: every
set of kinds files each kind's bytes where that kind alone does.

The jobs of the kinds' own test files have 3 channels and a window of 2, so a step never comes down in four pieces.  This one is the
smallest that does, with more than one kind riding behind the last of the four: 8 channels, 8 blocks, window 4 (steps of 4 blocks, 8 and
more encoded rows), LPCM24 out, dither on, a short power amp on channel 1, an overdrive on channel 2, the metronome into the master.
Sharded 7 + 1, the 7-channel shard runs the metronome: 8 encoded rows, and its 3 float64 rows share the last piece with the sections.

All comparisons are byte equality between runs with different switch sets; the numbers of each kind are its own test file's business."""
from itertools import combinations

import numpy as np
import pytest

from helpers import package

pytestmark = pytest.mark.gpu

BLOCK, RATE = 8192, 48000
NCH, BLOCKS, WINDOW = 8, 8, 4
KINDS = ("report", "spectrum", "align", "true_peak")
FIR = np.array([0.0, 0.0, 0.0, 0.0, 0.0, -0.9, 0.1])
EDGES = [100.0, 1000.0, 10000.0]                                     # two bands: 16 bytes per port and block
# port p against port REFS[p] (-1: not measured): the plain call's N + 3 ports; a shard's chain outputs and the metronome
REFS = {(0, NCH, False): [-1, 0, 0, 2, -1, 4, 0, 6, 0, 8, 1], (0, 7, True): [-1, 0, 0, 2, -1, 4, 0, 1], (7, 1, True): [0, -1]}
_job = {}


def the_job():
    if _job:
        return _job
    n = BLOCKS * BLOCK
    rng = np.random.default_rng(12)
    t = np.arange(n) / RATE
    enc = lambda x: np.frombuffer(np.asarray(x, dtype="<f8").tobytes(), dtype=np.uint8)
    inputs = [enc(0.4 * np.sin(2 * np.pi * 110.0 * (c + 1) * t) + 0.05 * rng.uniform(-1, 1, n)) for c in range(NCH)]
    _job.update(inputs=[(x, "ieee64", RATE) for x in inputs], length=n,
                tick=0.008 * np.sin(np.arange(600) * 0.2), tock=0.006 * np.sin(np.arange(400) * 0.3))
    return _job


def configured(kinds, first=0, count=NCH, shard=False):
    pkg, job = package(), the_job()
    ctx = pkg.Context(count, BLOCK)
    if first <= 1 < first + count:
        ctx.append_unit(1 - first, "power_amp", fir=FIR)
    if first <= 2 < first + count:
        ctx.append_unit(2 - first, "overdrive", params=[0, 15, 80, -3, 1, 0])
    ctx.spatializer_set_sample_rate(RATE)
    for c in range(count):
        ctx.spatializer_set_position(c, -60.0 + 15.0 * (first + c), 0.7, 1.0 - 0.05 * (first + c))
    ctx.metronome_set_sounds(job["tick"], job["tock"])
    ctx.metronome_configure(3, 200, RATE)
    ctx.set_window(WINDOW)
    ctx.batch_set_dither(1, seed=99, port_base=first)
    if "report" in kinds:
        ctx.batch_report_enable()
    if "spectrum" in kinds:
        ctx.batch_spectrum_enable(EDGES)
    if "align" in kinds:
        ctx.batch_align_enable(REFS[(first, count, shard)], 64)
    if "true_peak" in kinds:
        ctx.batch_true_peak_enable()
    return ctx


def records(ctx, kind):
    return {"report": ctx.batch_report, "spectrum": ctx.batch_spectrum, "align": ctx.batch_align, "true_peak": ctx.batch_true_peak}[kind]().tobytes()


# ---- the plain call ------------------------------------------------------------------------------------------------------------------
def plain_run(kinds):
    ctx = configured(kinds)
    outs = [o.tobytes() for o in ctx.batch_run(the_job()["inputs"], RATE, "lpcm24", metronome_to_master=True)]
    recs = {k: records(ctx, k) for k in kinds}
    ctx.close()
    return outs, recs


@pytest.fixture(scope="module")
def plain_alone():
    package().build()
    outs, _ = plain_run(())
    alone = {}
    for k in KINDS:
        o, r = plain_run((k,))
        assert o == outs, "%s changes no output byte" % k
        alone[k] = r[k]
    sizes = {"report": 32, "spectrum": 8 * (len(EDGES) - 1), "align": 40, "true_peak": 16}
    for k in KINDS:
        assert len(alone[k]) == (NCH + 3) * BLOCKS * sizes[k] and any(alone[k]), k
    return outs, alone


@pytest.mark.parametrize("kinds", [KINDS] + list(combinations(KINDS, 2)), ids="+".join)
def test_plain_call_every_kind_equals_itself_alone(plain_alone, kinds):
    outs, alone = plain_alone
    o, r = plain_run(kinds)
    assert o == outs, "the kinds change no output byte"
    for k in kinds:
        assert r[k] == alone[k], "%s beside %s" % (k, "+".join(kinds))


# ---- the sharded call: 7 + 1 channels, slices of 4 blocks, the master finished per slice on the small shard's context -----------------------
def sharded_run(kinds):
    """per slice: every context's records of every kind, the finish's two rows of every kind but the alignment records, and all the bytes"""
    pkg, job = package(), the_job()
    shards = ((0, 7), (7, 1))
    ctxs = [configured(kinds, f, n, shard=True) for f, n in shards]
    gens = [c.batch_stream_shard(job["inputs"][f:f + n], RATE, "lpcm24", 4, job_samples=job["length"], metronome=(g == 0))
            for g, (c, (f, n)) in enumerate(zip(ctxs, shards))]
    slices = []
    for _ in range(BLOCKS // 4):
        parts = [next(gen) for gen in gens]
        here = {"shard": [{k: records(c, k) for k in kinds} for c in ctxs]}
        here["bytes"] = [o.tobytes() for p in parts for o in p[0]] + [parts[0][3].tobytes()] + [p[s].tobytes() for p in parts for s in (1, 2)] + [parts[0][4].tobytes()]
        ml, mr = ctxs[1].batch_finish_master_slice("lpcm24", [p[1] for p in parts], [p[2] for p in parts], aux=parts[0][4], sample_rate=RATE)
        here["bytes"] += [ml.tobytes(), mr.tobytes()]
        here["finish"] = {k: records(ctxs[1], k) for k in kinds if k != "align"}
        if "align" in kinds:
            with pytest.raises(pkg.GdgError, match="no alignment records"):
                ctxs[1].batch_align()
        slices.append(here)
    for gen in gens:
        assert next(gen, None) is None
    for c in ctxs:
        c.close()
    return slices


def test_sharded_call_every_kind_equals_itself_alone():
    package().build()
    none = sharded_run(())
    four = sharded_run(KINDS)
    sizes = {"report": 32, "spectrum": 8 * (len(EDGES) - 1), "align": 40, "true_peak": 16}
    for k in KINDS:
        alone = sharded_run((k,))
        for s, (a, b, z) in enumerate(zip(alone, four, none)):
            assert a["bytes"] == z["bytes"] and b["bytes"] == z["bytes"], "slice %d: the kinds change no output byte" % s
            for g in range(2):
                assert b["shard"][g][k] == a["shard"][g][k] and any(b["shard"][g][k]), "slice %d, shard %d: %s beside the other three" % (s, g, k)
            assert len(b["shard"][0][k]) == 8 * 4 * sizes[k] and len(b["shard"][1][k]) == 2 * 4 * sizes[k]
            # the metronome row of the shard that does not run it: all zero bytes
            assert b["shard"][1][k][4 * sizes[k]:] == bytes(4 * sizes[k]), "slice %d: %s, the metronome row of the shard without it" % (s, k)
            if k != "align":
                assert b["finish"][k] == a["finish"][k] and len(b["finish"][k]) == 2 * 4 * sizes[k] and any(b["finish"][k]), "slice %d: the finish's %s" % (s, k)
