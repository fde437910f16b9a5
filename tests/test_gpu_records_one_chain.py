"""The nine things a batch call can keep beside its files -- the render report's four kinds (statistics, band spectrum, alignment, true peak)
and the five list records (blend fit, Gram list, tap fit, transfer records, the delivered rows' records) -- ride one layout behind a step's rows
(csrc/report_sections.h): the four kinds' sections, then the one chain of the five.  What holds that layout: on a streamed job of 2 channels
at 48 kHz, 5 blocks cut into slices of 3 and 2 blocks in windows of 4 (steps of 2, 1, 1 and 1 blocks: sections of differing widths, and every
carried history crosses the slice boundary), delivered at a half of the rate and 147/160 of that, with one blend that reaches back, all nine
at once give, byte for byte, what each gives alone, and every run writes the same files.  And two refusals in their standing words: the
buffers of an open job cannot be released between two slices -- which is what keeps the four carried histories, so the refusal that a history
"of the open job is gone" has no way to be provoked through the calls and is pinned as text (tests/test_list_records_host.py) -- and a shard
cannot be opened with a transfer list in force."""
import numpy as np
import pytest

from helpers import package, synth_signal

pytestmark = pytest.mark.gpu

BLOCK = 8192
RATE, NCH, BLOCKS, WINDOW = 48000, 2, 5, 4
SLICES = (3, 2)
SAMPLES = (BLOCKS - 1) * BLOCK + 1000
NO = NCH + 3
NR = NO + 1
DELIVERY = (2, 147, 160)
BLENDS = [[(0, 0.6, 37), (1, -0.4)]]                                            # port NO; its first term reads 37 samples back
KINDS = {                                                                       # kind -> (what switches it on, its getter)
    "stats": (lambda ctx: ctx.batch_report_enable(True), "batch_report"),
    "spectrum": (lambda ctx: ctx.batch_spectrum_enable([100.0, 1000.0, 5000.0, 20000.0]), "batch_spectrum"),      # 3 bands
    "align": (lambda ctx: ctx.batch_align_enable([-1, 0, -1, -1, -1, 0], 64), "batch_align"),
    "true_peak": (lambda ctx: ctx.batch_true_peak_enable(True), "batch_true_peak"),
    "fit": (lambda ctx: ctx.batch_fit_enable([(NO, [0, 1])]), "batch_fit"),
    "gram": (lambda ctx: ctx.batch_gram_enable([0, NCH, NO]), "batch_gram"),
    "tapfit": (lambda ctx: ctx.batch_tapfit_enable([(0, [1], 4)]), "batch_tapfit"),
    "transfer": (lambda ctx: ctx.batch_transfer_enable([(0, 1)], 32), "batch_transfer"),
    "delivered": (lambda ctx: ctx.batch_delivered_enable(True), "batch_delivered"),
}


def lpcm16_file(x):
    return np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)


class Job:
    def __init__(self):
        self.pkg = package()
        self.inputs = [(lpcm16_file(0.5 * synth_signal(c, SAMPLES, RATE)), "lpcm16", RATE) for c in range(NCH)]
        self.metas = [(SAMPLES, "lpcm16", RATE)] * NCH
        self.cache = {}

    def configured(self, on, delivery=DELIVERY, blends=BLENDS):
        ctx = self.pkg.Context(NCH, BLOCK)
        ctx.append_unit(0, "overdrive", params=[0, 20, 100, 0, 1, 2])
        ctx.append_unit(1, "tone_stack")
        ctx.spatializer_set_sample_rate(RATE)
        for c in range(NCH):
            ctx.spatializer_set_position(c, -40.0 + 80.0 * c, 1.0 + 0.5 * c, 0.8)
        ctx.set_window(WINDOW)
        ctx.batch_set_blends(blends)
        if delivery:
            ctx.batch_set_delivery_ratio(*delivery)
        for kind in on:
            KINDS[kind][0](ctx)
        return ctx

    def run(self, on, release_between=False):
        """-> (the files, {kind: its getter's bytes behind every slice}) of the job with the kinds `on`"""
        key = tuple(on)
        if key in self.cache:
            return self.cache[key]
        ctx = self.configured(on)
        left = list(SLICES)
        pieces, records = [], {kind: [] for kind in on}
        for outs in ctx.batch_stream(self.inputs, RATE, "lpcm24", lambda _left: left.pop(0)):
            pieces.append([o.tobytes() for o in outs])
            for kind in on:
                records[kind].append(getattr(ctx, KINDS[kind][1])().tobytes())
            if release_between and left:
                with pytest.raises(self.pkg.GdgError, match="a streamed batch run is open on this context: its buffers are in use") as e:
                    ctx.batch_release()
                assert e.value.code == self.pkg.GDG_ERR_INVALID
        ctx.close()
        assert len(pieces) == len(SLICES) and all(len(p) == NR for p in pieces)
        files = [b"".join(p[r] for p in pieces) for r in range(NR)]
        self.cache[key] = (files, records)
        return self.cache[key]


@pytest.fixture(scope="module")
def job():
    return Job()


def test_all_nine_at_once_are_each_alone_and_every_run_writes_the_same_files(job):
    """... and the release that is refused between run A's two slices leaves its histories where they are: run A is the runs B"""
    files_a, rec_a = job.run(tuple(KINDS), release_between=True)
    assert all(f.strip(b"\0") for f in files_a[:NCH] + files_a[NO:]) and len({len(f) for f in files_a}) == 1
    for kind in KINDS:
        files_b, rec_b = job.run((kind,))
        assert len(rec_a[kind]) == len(rec_b[kind]) == len(SLICES) and all(r.strip(b"\0") for r in rec_a[kind]), kind
        for s, (a, b) in enumerate(zip(rec_a[kind], rec_b[kind])):
            assert a == b, "%s, slice %d: all nine on against alone" % (kind, s)
        for r in range(NR):
            assert files_b[r] == files_a[r], (kind, r)


def test_a_shard_refuses_the_transfer_list_in_its_standing_words(job):
    pkg = job.pkg
    ctx = job.configured(("transfer",), delivery=None, blends=None)              # which the shard calls refuse first
    with pytest.raises(pkg.GdgError, match="gdg_batch_stream_open_shard: 1 transfer pairs are in force on this context \\(gdg_batch_transfer_enable\\); "
                                           "a sharded job cannot collect transfer records yet") as e:
        ctx.batch_stream_open_shard(job.metas, RATE, "lpcm24")
    assert e.value.code == pkg.GDG_ERR_UNSUPPORTED
    ctx.close()
