"""The chorus's output bits, leg by leg, saved for a comparison between two builds (profiles/chorus_one_text.txt):

    python profiles/probes/chorus_bits.py OUT.npz            # once per build, each in its own process
    python profiles/probes/chorus_bits.py --compare A.npz B.npz

Every leg runs a two-channel context with a chorus on each channel: channel 1 takes the setting of the 192 kHz chorus case of
tests/lfo_delay_ref.py (depth 100, speed 100: robust whole delays at call 6, sample 6400 and call 20, sample 0), channel 0 lfo_delay_ref.QUIET.
Legs:
  - 8192 frames at 192 kHz, 22 calls (past both hits; the ring of 32768 cells wraps five times) in SEGT (the defaults), GENERAL
    (seg_tile_max_channels = 0) and SEGF (seg_two_per_cu_min_channels = 2);
  - the same stream in windows of 4 (WAVE), 24 frames, at 192 kHz (a frame may append while the one before still reads) and at 96 kHz (it may not);
  - 1000 and then 999 frames at 48 kHz in GENERAL, 12 calls each: the even size appends in pairs; after the first odd call the write position
    is odd, so the single-cell append runs, and every thread's pair of samples is a pair of one.
The launch shapes that ran are printed per leg (GDG_PLAN_TRACE=2)."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WINDOW = 4


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), (a.files, b.files)
    ok = True
    for leg in a.files:
        same = np.array_equal(a[leg], b[leg])
        ok &= same
        print("%-24s %-28s %s" % (leg, a[leg].shape, "equal" if same else "DIFFERS: max |a - b| %.3e" % float(np.abs(a[leg] - b[leg]).max())))
    return 0 if ok else 1


def main(out_path):
    os.environ["GDG_PLAN_TRACE"] = "2"
    import __graft_entry__ as entry
    import lfo_delay_ref as ref
    pkg = entry.load_package()
    case = next(c for c in ref.CASES if c.unit == "chorus" and c.sr == 192000)
    blocks = ref.block_inputs(ref.case_seed(case), 8192)

    def context(frames, options=()):
        ctx = pkg.Context(2, frames)
        for key, v in options:
            ctx.set_option(key, v)
        ctx.append_unit(0, "chorus", params=ref.QUIET["chorus"])
        ctx.append_unit(1, "chorus", params=case.params)
        return ctx

    legs = {}
    for name, options in (("frames_192k_segt", ()), ("frames_192k_general", (("seg_tile_max_channels", 0),)),
                          ("frames_192k_segf", (("seg_two_per_cu_min_channels", 2),))):
        ctx = context(8192, options)
        legs[name] = np.stack([ctx.process(np.stack([blocks[b % 4], blocks[b % 4]]), 192000) for b in range(22)], axis=1)
        ctx.close()
        print("leg %s done" % name, file=sys.stderr, flush=True)
    for sr in (192000, 96000):
        calls = 24
        ctx = context(8192)
        ctx.set_window(WINDOW)
        row = np.concatenate([blocks[b % 4] for b in range(calls)])
        d_in, d_out = ctx.alloc(2, row.size), ctx.alloc(2, row.size)
        d_in.upload(np.stack([row, row]))
        for b in range(0, calls, WINDOW):
            ctx.process_window_device(d_in.ptr + 8 * b * 8192, d_out.ptr + 8 * b * 8192, row.size, WINDOW, sr)
            ctx.synchronize()
        legs["windows_%dk" % (sr // 1000)] = d_out.download().reshape(2, calls, 8192)
        ctx.close()
        print("leg windows %d done" % sr, file=sys.stderr, flush=True)
    ctx = context(1000)
    small = ref.block_inputs(4321, 1000)
    out = []
    for b in range(24):
        n = 1000 if b < 12 else 999
        out.append(ctx.process(np.stack([small[b % 4, :n], small[(b + 1) % 4, :n]]), 48000))
    ctx.close()
    legs["frames_48k_1000"] = np.stack(out[:12], axis=1)
    legs["frames_48k_999"] = np.stack(out[12:], axis=1)
    print("leg 48 kHz done", file=sys.stderr, flush=True)
    for name, v in legs.items():
        assert np.isfinite(v).all(), name
    np.savez(out_path, **legs)
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(main(sys.argv[1]))
