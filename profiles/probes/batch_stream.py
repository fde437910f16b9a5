"""The streamed batch run beside the one-call run: the bench's batch job -- 512 16-bit files in, 24-bit files out,
W = 16, two 65536-tap amps -- as one gdg_batch_run, streamed in slices of 32 / 64 / 128 blocks, and the same slices fed as separate
gdg_batch_run calls (what a caller can do by hand for same-rate mono files).  Every figure is the median of `--reps` runs with the
smallest and the largest beside it: the spread of repeated runs is what a difference has to exceed.  All calls are timed at the C
boundary, arguments marshalled before the clock starts.

    python profiles/probes/batch_stream.py [--blocks 512] [--reps 5] > profiles/batch_stream.txt
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import bench  # noqa: E402

BLOCK = 8192


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2] * 1e3, ts[0] * 1e3, ts[-1] * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=512)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    pkg = entry.load_package()
    lib = pkg.lib()
    nch, sr, blocks = args.channels, 192000, args.blocks
    ctx = bench.make_context(pkg, nch, BLOCK, 0, 65536)
    ctx.set_window(16)
    files = bench.batch_files(nch, sr, blocks)
    samples = nch * blocks * BLOCK
    print("job: %d files x %d blocks, lpcm16 in, lpcm24 out, W = 16, %d reps per figure (median, min .. max)" % (nch, blocks, args.reps))

    def report(name, ts, extra=""):
        med, lo, hi = stats(ts)
        print("%-44s %9.2f ms  (%8.2f .. %8.2f)  %6.2f Gsamples/s  %s" % (name, med, lo, hi, samples / med / 1e6, extra))

    # ---- one call ---------------------------------------------------------------------------------------------------------------------
    call, outs = ctx.batch_prepared(files, sr, "lpcm24")
    call()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
    one_kib = ctx.get_option("stat_batch_device_kib")
    report("one gdg_batch_run", ts, "device buffers %.1f MiB" % (one_kib / 1024))
    want = [o.copy() for o in outs[:2]] + [outs[nch].copy()]
    ctx.batch_release()

    # ---- the same slices: streamed, and as separate gdg_batch_run calls ------------------------------------------------------------
    opt = pkg.BatchOptions(sr, pkg.WAVE_FORMATS["lpcm24"], 0, 0, 0)
    for per in (32, 64, 128):
        if per > blocks:
            continue
        n_slices = blocks // per
        out_ptrs = [(C.c_void_p * (nch + 3))(*[o.ctypes.data + s * per * BLOCK * 3 for o in outs]) for s in range(n_slices)]
        in_ptrs = [(C.c_void_p * nch)(*[f[0].ctypes.data + s * per * BLOCK * 2 for f in files]) for s in range(n_slices)]
        metas = [(blocks * BLOCK, "lpcm16", sr)] * nch
        ts = []
        for rep in range(args.reps + 1):
            ctx.batch_stream_open(metas, sr, "lpcm24")
            t0 = time.perf_counter()
            for s in range(n_slices):
                ctx._check(lib.gdg_batch_stream_step(ctx._h, per, in_ptrs[s], out_ptrs[s]))
            dt = time.perf_counter() - t0
            ctx.batch_stream_close()
            if rep:
                ts.append(dt)
        kib = ctx.get_option("stat_batch_device_kib")
        report("streamed, slices of %d blocks" % per, ts, "device buffers %.1f MiB" % (kib / 1024))
        if per == 32:
            # the bytes are the one-call run's up to the units' state, which carries over from run to run: compare shapes only here; the
            # tests compare bytes on fresh contexts
            assert all(o.size == w.size for o, w in zip(outs[:2] + [outs[nch]], want))
        ctx.batch_release()
        arrs = []
        for s in range(n_slices):
            arr = (pkg.BatchInput * nch)()
            for c, f in enumerate(files):
                arr[c] = pkg.BatchInput(f[0].ctypes.data + s * per * BLOCK * 2, per * BLOCK, pkg.WAVE_FORMATS["lpcm16"], sr, 1, 0)
            arrs.append(arr)
        ts = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            for s in range(n_slices):
                ctx._check(lib.gdg_batch_run(ctx._h, arrs[s], nch, C.byref(opt), out_ptrs[s]))
            dt = time.perf_counter() - t0
            if rep:
                ts.append(dt)
        kib = ctx.get_option("stat_batch_device_kib")
        report("separate gdg_batch_run calls of %d blocks" % per, ts, "device buffers %.1f MiB" % (kib / 1024))
        ctx.batch_release()
    ctx.close()


if __name__ == "__main__":
    main()
