#!/usr/bin/env python3
"""The master mix of a sharded job, timed once per entry point: gdg_batch_finish_master and gdg_batch_finish_master_slice share ONE engine
(finish_master, api_batch.cpp), so the two rows of a size are two series of the same code and their difference is noise -- the probe no
longer compares two implementations.  Run on a commit where the whole-job finish still had a loop of its own, the rows are that loop and
the engine; that is how profiles/finish_master_one_engine.txt was made.
On the same host arrays: G = 8, lpcm24, aux, meters off, 4, 16 and 64 blocks; host wall-clock of the C call alone, the entry points
alternated in one process, 5 warm-up calls and 25 measured calls each.
Then, for information, one 3-context job of tests/test_gpu_batch_stream.py's _long_job: the streamed sharded run beside the one-call
sharded run (one device carries all three shards: it says nothing about a job over several GPUs); --finish-only leaves it out.
Usage: finish_master_slice.py [--finish-only] [output file]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry

BLOCK = 8192


def stats(v):
    v = np.sort(np.asarray(v)) * 1e3
    return "median %8.3f  min %8.3f  max %8.3f  p25 %8.3f  p75 %8.3f" % (np.median(v), v[0], v[-1], v[len(v) // 4], v[(3 * len(v)) // 4])


def finish_times(pkg, lines):
    G, fmt, rate, warm, reps = 8, pkg.WAVE_FORMATS["lpcm24"], 48000, 5, 25
    lib = pkg.lib()
    ctx = pkg.Context(1, BLOCK)
    rng = np.random.default_rng(1)
    lines.append("the finish: G = %d, lpcm24, aux, meters off; ms per call (host wall-clock), %d calls after %d warm-up calls, the entry points alternated" % (G, reps, warm))
    entries = {"gdg_batch_finish_master": lib.gdg_batch_finish_master, "gdg_batch_finish_master_slice": lib.gdg_batch_finish_master_slice}
    for blocks in (4, 16, 64):
        n = blocks * BLOCK
        lefts = [rng.uniform(-0.2, 0.2, n) for _ in range(G)]
        rights = [rng.uniform(-0.2, 0.2, n) for _ in range(G)]
        aux = rng.uniform(-0.2, 0.2, n)
        lp = (C.c_void_p * G)(*[a.ctypes.data for a in lefts])
        rp = (C.c_void_p * G)(*[a.ctypes.data for a in rights])
        outs = {name: (np.zeros(n * 3, dtype=np.uint8), np.zeros(n * 3, dtype=np.uint8)) for name in entries}
        times = {name: [] for name in entries}
        for i in range(warm + reps):
            for name, call in entries.items():
                ml, mr = outs[name]
                t0 = time.perf_counter()
                rc = call(ctx._h, fmt, lp, rp, G, aux.ctypes.data, n, rate, 0, ml.ctypes.data, mr.ctypes.data)
                dt = time.perf_counter() - t0
                assert rc == 0, (name, rc)
                if i >= warm:
                    times[name].append(dt)
        a, b = outs.values()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "the two entry points differ"
        for name in entries:
            lines.append("  %2d blocks  %-30s %s" % (blocks, name, stats(times[name])))
    ctx.close()


def job_ab(pkg, lines):
    import test_gpu_batch_stream as tbs
    orc = entry.load_oracle()
    orc.build()
    rate, inputs, _ = tbs._long_job(orc, pkg)
    from helpers import synth_ir
    split = [(0, 2), (2, 1), (3, 1)]                                # its four channels as 2 + 1 + 1
    irs = [synth_ir(2500, seed=70 + c) for c in range(4)]

    def contexts():
        ctxs = []
        for first, count in split:
            ctx = pkg.Context(count, BLOCK)
            for c in range(count):
                for name, p in tbs.CHAIN:
                    ctx.append_unit(c, name, fir=irs[first + c]) if p == "ir" else ctx.append_unit(c, name, params=p)
            ctx.spatializer_set_sample_rate(rate)
            ctx.metronome_set_sounds(np.linspace(-0.5, 0.5, 800), np.linspace(0.4, -0.4, 500))
            ctx.metronome_configure(4, 150, rate)
            ctx.set_window(4)
            ctxs.append(ctx)
        return ctxs

    job = 41 * BLOCK

    def one_call(ctxs):
        sh = [ctx.batch_run_shard(inputs[f:f + n], rate, "lpcm24", job_samples=job, metronome=(g == 0)) for g, (ctx, (f, n)) in enumerate(zip(ctxs, split))]
        return ctxs[0].batch_finish_master("lpcm24", [s[1] for s in sh], [s[2] for s in sh], aux=sh[0][4])

    def streamed(ctxs):
        gens = [ctx.batch_stream_shard(inputs[f:f + n], rate, "lpcm24", 8, job_samples=job, metronome=(g == 0)) for g, (ctx, (f, n)) in enumerate(zip(ctxs, split))]
        out = []
        for parts in zip(*gens):
            out.append(ctxs[0].batch_finish_master_slice("lpcm24", [p[1] for p in parts], [p[2] for p in parts], aux=parts[0][4]))
        for gen in gens:
            gen.close()
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])

    lines.append("")
    lines.append("one job of 41 blocks, 4 channels on 3 contexts of ONE device, window 4, shards one after the other on one thread (Python); ms per job, second of two runs")
    res = {}
    for name, fn in (("one-call shards + gdg_batch_finish_master", one_call), ("slices of 8 blocks + gdg_batch_finish_master_slice", streamed)):
        ctxs = contexts()
        fn(ctxs)
        for ctx in ctxs:
            ctx.close()
        ctxs = contexts()
        t0 = time.perf_counter()
        res[name] = fn(ctxs)
        dt = time.perf_counter() - t0
        for ctx in ctxs:
            ctx.close()
        lines.append("  %-52s %9.1f" % (name, dt * 1e3))
    a, b = res.values()
    lines.append("  master bytes equal: %s" % bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])))


def main():
    pkg = entry.load_package()
    args = [a for a in sys.argv[1:] if a != "--finish-only"]
    lines = []
    finish_times(pkg, lines)
    if "--finish-only" not in sys.argv[1:]:
        job_ab(pkg, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if args:
        with open(args[0], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
