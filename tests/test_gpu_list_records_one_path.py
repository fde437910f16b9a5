"""The three list records of a batch call -- blend fit, Gram list, tap fit -- ride one path (csrc/report_sections.h, LIST_KINDS): their
sections are chained behind the render report's, filed by one rule and launched from one table.  What holds that path, on test_gpu_tapfit's
job (3 channels on one source, 1 blend, 3 blocks of 8192, report on) with one 2-term fit, a 3-port Gram list and one K = 1, T = 4 tap fit:
all three at once give, bit for bit, what each gives alone and what the stand-alone calls give on the call's own IEEE64 files; the same bytes
whatever the window and the slicing; every on/off subset leaves outputs and block statistics alone and is counted byte by byte; one context
takes several lists in turn as a fresh one would; and the shard calls refuse the kinds in their order."""
import itertools

import numpy as np
import pytest

from helpers import package, synth_ir, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
RATE, NCH, BLOCKS = 48000, 3, 3
SAMPLES = 2 * BLOCK + 1000
NO = NCH + 3
BLENDS = [[(0, 0.6), (1, -0.3)]]                                                # port NO
FIT = [(NO, [0, 1])]                                                            # one 2-term fit, the blend port its target
GRAM = [0, NCH, NO]                                                             # a chain output, master left, the blend port
TAPFIT = [(0, [1], 4)]                                                          # K = 1, T = 4: 5 virtual rows, 15 doubles
TAPFIT_LARGER = [(NO, [0, 2], 8)]                                               # K = 2, T = 8: 17 virtual rows, 153 doubles
KINDS = ("fit", "gram", "tapfit")
ALL = dict(fit=FIT, gram=GRAM, tapfit=TAPFIT)


def tapfit_doubles(fits):
    return sum((len(ports) * taps + 1) * (len(ports) * taps + 2) // 2 for _, ports, taps in fits)


def grown_bytes(lists, window):
    """what a kind in force adds to the batch buffers: its table of ints, and in each of the two download halves 16 bytes and a window of
    its elements -- [fits] records of 368 bytes (10 ints per fit), P (P + 1) / 2 doubles (P ints), D doubles (9 ints per fit)"""
    fit, gram, tapfit = lists.get("fit") or [], lists.get("gram") or [], lists.get("tapfit") or []
    total = 0
    if fit:
        total += 4 * 10 * len(fit) + 2 * (16 + len(fit) * window * 368)
    if gram:
        total += 4 * len(gram) + 2 * (16 + window * (len(gram) * (len(gram) + 1) // 2) * 8)
    if tapfit:
        total += 4 * 9 * len(tapfit) + 2 * (16 + window * tapfit_doubles(tapfit) * 8)
    return total


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


def same(got, want, what):
    """records of any of the three kinds, byte for byte"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    a, b = np.frombuffer(got.tobytes(), np.uint8), np.frombuffer(want.tobytes(), np.uint8)
    wrong = np.flatnonzero(a != b)
    assert wrong.size == 0, "%s: %d of %d bytes differ, the first at %d" % (what, wrong.size, a.size, wrong[0])


class Job:
    """test_gpu_tapfit's: 3 channels on one source with power amps of different random taps"""

    def __init__(self):
        self.pkg = package()
        self.file = lpcm16_file(0.1 * synth_signal(0, SAMPLES, RATE) + 0.2 * np.random.default_rng(11).uniform(-1.0, 1.0, SAMPLES))
        self.inputs = [(self.file, "lpcm16", RATE)] + [None] * (NCH - 1)
        self.metas = [(SAMPLES, "lpcm16", RATE)] + [None] * (NCH - 1)
        self.irs = [synth_ir(n, seed=730 + c) for c, n in enumerate((300, 64, 128))]
        self.cache = {}

    @staticmethod
    def enable(ctx, lists):
        """lists: kind -> list; a kind that is missing is never mentioned to the context, an empty list switches it off"""
        for kind in KINDS:
            if kind in lists:
                getattr(ctx, "batch_%s_enable" % kind)(lists[kind])

    def configured(self, window, lists):
        ctx = self.pkg.Context(NCH, BLOCK)
        for c in range(NCH):
            ctx.append_unit(c, "power_amp", fir=self.irs[c])
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(NCH):
            ctx.spatializer_set_position(c, -60.0 + 30.0 * c, 1.0 + 0.25 * c, 0.8)
        ctx.set_window(window)
        ctx.batch_set_sources([0] * NCH)
        ctx.batch_set_blends(BLENDS)
        ctx.batch_report_enable(True)
        self.enable(ctx, lists)
        return ctx

    @staticmethod
    def records(ctx, lists):
        return {kind: getattr(ctx, "batch_%s" % kind)() for kind in KINDS if lists.get(kind)}

    def job_of(self, ctx, lists):
        outs = ctx.batch_run(self.inputs, RATE, "ieee64")
        return dict(outs=outs, rec=self.records(ctx, lists), report=ctx.batch_report(), kib=ctx.get_option("stat_batch_device_kib"))

    def run(self, window, lists, jobs=1):
        """the last of `jobs` jobs of a fresh context configured with `lists` from the start"""
        key = (window, repr(sorted(lists.items())), jobs)
        if key not in self.cache:
            ctx = self.configured(window, lists)
            for _ in range(jobs):
                got = self.job_of(ctx, lists)
            ctx.close()
            self.cache[key] = got
        return self.cache[key]


@pytest.fixture(scope="module")
def job():
    return Job()


def same_outputs(got, want, what):
    assert len(got["outs"]) == len(want["outs"]) == NO + 1
    for r in range(NO + 1):
        assert np.array_equal(got["outs"][r], want["outs"][r]), (what, r)
    assert got["report"].tobytes() == want["report"].tobytes(), what


def test_all_three_at_once_are_each_alone_and_the_stand_alone_calls(job):
    run = job.run(2, ALL)
    rows = np.stack([o.view(np.float64) for o in run["outs"]])
    assert rows.shape == (NO + 1, BLOCKS * BLOCK) and np.isfinite(rows).all() and all(r.any() for r in rows[:NCH])
    assert run["rec"]["fit"].shape == (1, BLOCKS) and run["rec"]["gram"].shape == (BLOCKS, 6) and run["rec"]["tapfit"].shape == (BLOCKS, 15)
    assert all(run["rec"][kind].tobytes().strip(b"\0") for kind in KINDS)
    for kind in KINDS:
        same(run["rec"][kind], job.run(2, {kind: ALL[kind]})["rec"][kind], "%s: all on against alone" % kind)
    ctx1 = job.pkg.Context(1, BLOCK)
    alone = dict(fit=ctx1.block_fit(rows, FIT, BLOCK), gram=ctx1.block_gram(rows, GRAM, BLOCK), tapfit=ctx1.block_tapfit(rows, TAPFIT, BLOCK))
    ctx1.close()
    for kind in KINDS:
        same(run["rec"][kind], alone[kind], "%s: batch against stand-alone" % kind)


def test_the_same_bytes_however_the_job_is_cut(job):
    """windows 1, 2 and 16 (steps of 1 + 1 + 1, 2 + 1 and 2 + 1 blocks: a tail behind the whole window) and slices of 1 + 2 and 2 + 1 blocks"""
    want = job.run(1, ALL)["rec"]
    for window in (2, 16):
        got = job.run(window, ALL)["rec"]
        for kind in KINDS:
            same(got[kind], want[kind], "%s: window %d against window 1" % (kind, window))
    for cuts in ((1, 2), (2, 1)):
        ctx = job.configured(2, ALL)
        parts = []
        for _ in ctx.batch_stream(job.inputs, RATE, "ieee64", lambda left: cuts[0] if left == BLOCKS else cuts[1]):
            parts.append(job.records(ctx, ALL))
        ctx.close()
        assert [p["gram"].shape[0] for p in parts] == list(cuts) and [p["fit"].shape[1] for p in parts] == list(cuts)
        for kind in KINDS:                                                      # the fits' blocks run along a record row, the others' down the rows
            same(np.concatenate([p[kind] for p in parts], axis=1 if kind == "fit" else 0), want[kind], "%s: slices of %d + %d" % ((kind,) + cuts))


@pytest.mark.parametrize("on", [s for n in range(4) for s in itertools.combinations(KINDS, n)], ids=lambda s: "+".join(s) or "none")
def test_every_subset_changes_no_output_byte_and_is_counted(job, on):
    """the kinds that are not `on` are switched off with an empty list; `never` is a context that was told of none of them"""
    never = job.run(2, {})
    lists = {kind: ALL[kind] if kind in on else [] for kind in KINDS}
    got = job.run(2, lists)
    same_outputs(got, never, on)
    assert sorted(got["rec"]) == sorted(on)
    for kind in on:
        same(got["rec"][kind], job.run(2, ALL)["rec"][kind], "%s of %s against all on" % (kind, on))
    # the tables and the rooms of the kinds that are on, those of each alone added up; the option counts whole KiB
    grown = grown_bytes(lists, 2)
    assert grown == sum(grown_bytes({kind: ALL[kind]}, 2) for kind in on)
    assert grown // 1024 <= got["kib"] - never["kib"] <= -(-grown // 1024), (got["kib"], never["kib"], grown)
    if not on:
        assert got["kib"] == never["kib"]


def test_one_context_takes_several_lists_in_turn(job):
    pkg = job.pkg
    turns = [ALL, dict(fit=FIT, gram=[], tapfit=TAPFIT_LARGER), dict(fit=[], gram=[], tapfit=[])]
    ctx = job.configured(2, turns[0])
    for n, lists in enumerate(turns):
        job.enable(ctx, lists)
        got = job.job_of(ctx, lists)
        want = job.run(2, lists, jobs=n + 1)                                    # job n + 1 of a context: the units go on where the job before left them
        same_outputs(got, want, "turn %d" % n)
        assert sorted(got["rec"]) == sorted(want["rec"]) == sorted(kind for kind in KINDS if lists[kind])
        for kind in got["rec"]:
            same(got["rec"][kind], want["rec"][kind], "turn %d: %s" % (n, kind))
        assert got["kib"] == want["kib"], (n, got["kib"], want["kib"])
        if n == 0:
            # the kept difference: a fit record carries its own term count and outlives a re-enable of as many fits; the other two are
            # read with the list that made them
            ctx.batch_fit_enable(FIT)
            same(ctx.batch_fit(), got["rec"]["fit"], "fit records behind a re-enable")
            ctx.batch_gram_enable(GRAM)
            with pytest.raises(pkg.GdgError, match="no Gram records: .* none has run since gdg_batch_gram_enable") as e:
                ctx.batch_gram()
            assert e.value.code == pkg.GDG_ERR_INVALID
            ctx.batch_tapfit_enable(TAPFIT)
            with pytest.raises(pkg.GdgError, match="no tap-fit records: .* none has run since gdg_batch_tapfit_enable") as e:
                ctx.batch_tapfit()
            assert e.value.code == pkg.GDG_ERR_INVALID
    assert (ctx.batch_fits(), ctx.batch_gram_ports(), ctx.batch_tapfits()) == (0, [], 0)
    for kind, none in (("fit", "no fit records"), ("gram", "no Gram records"), ("tapfit", "no tap-fit records")):
        with pytest.raises(pkg.GdgError, match="%s: .* ran without them \\(gdg_batch_%s_enable comes before the call\\)" % (none, kind)) as e:
            getattr(ctx, "batch_%s" % kind)()
        assert e.value.code == pkg.GDG_ERR_INVALID
    ctx.close()
    assert job.run(2, turns[2], jobs=3)["kib"] == job.run(2, {})["kib"]             # off at last: the buffers of a context that never heard of them


def test_the_shard_calls_refuse_the_kinds_in_their_order(job):
    """fits, then the Gram list, then tap fits, each in its own words; nothing is launched by a refused call"""
    pkg = job.pkg
    ctx = job.configured(2, dict(fit=[(0, [1, 2])], gram=[0, 1, 2], tapfit=[(0, [1], 4)]))
    ctx.batch_set_blends([])                                                     # which the shard calls refuse first
    for off, what in ((None, "1 fits are in force on this context \\(gdg_batch_fit_enable\\); a sharded job cannot collect fit records yet"),
                      ("fit", "a Gram list of 3 ports is in force on this context \\(gdg_batch_gram_enable\\); a sharded job cannot collect Gram records yet"),
                      ("gram", "1 tap fits are in force on this context \\(gdg_batch_tapfit_enable\\); a sharded job cannot collect tap-fit records yet")):
        if off:
            job.enable(ctx, {off: []})
        for name, args in (("batch_run_shard", (job.inputs, RATE, "ieee64")), ("batch_stream_open_shard", (job.metas, RATE, "ieee64"))):
            with pytest.raises(pkg.GdgError, match="gdg_%s: %s" % (name, what)) as e:
                getattr(ctx, name)(*args)
            assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    ctx.close()
