#!/usr/bin/env python3
"""What the blend fit's records cost a batch run: bench.py's batch job (512 lpcm16 files of 128 blocks -> lpcm24, W = 16, 2 x 65536 taps,
192 kHz) in four forms -- the parent commit, this commit with fits off, this commit with 64 fits of two terms and with 64 fits of eight
terms -- ALTERNATING on one machine, every leg a fresh process under its own timeout.

The parent's tree, built, is expected beside this one:
    git worktree add .ab_parent HEAD^ && make -C .ab_parent/go-dsp-guitar_amd/csrc
(AB_PARENT names another place).  Without it the parent's legs are left out and the table says so.  The off leg is to be read against the
parent's, never against itself: it may differ from the parent's median by the spread of the parent's own process medians and no more.

    python profiles/probes/batch_fit.py [rounds]           -> the table on stdout and in profiles/batch_fit_ab.txt ($AB_OUT: elsewhere)

Odd rounds run "off" in front of "parent", so that neither always runs second.  A leg: 3 warm-up calls, then CALLS timed calls of the C
call alone (arguments marshalled once, as bench.py times it).  Per form the table gives the median over all timed calls of all rounds, the
fastest and slowest PROCESS median (the run-to-run spread) and the fastest call.  The fit legs also time the kernel alone on a buffer of
a step's shape -- 512 rows of 16 blocks, 64 fits, the stand-alone device entry (which uploads its table and waits, so the figure is an
upper bound of the kernel's time per step of the block loop) -- and print the sum of tt over the last call's records, so that a leg
that measured nothing shows."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CALLS, BLOCKS, SR, TAPS, W, NCH = 9, 128, 192000, 65536, 16, 512
N_FITS, KERNEL_REPS = 64, 20
LEG_TIMEOUT = 300                                        # seconds; a leg takes ~20 s, most of it the context's set-up
TERMS = {"two": 2, "eight": 8}


def fits_of(terms):
    """fit f: a target and `terms` term channels spread over the job"""
    return [((f * 8 + 3) % NCH, [(f * 8 + k * 61) % NCH for k in range(terms)]) for f in range(N_FITS)]


def child(root, form):
    sys.path.insert(0, root)
    import numpy as np
    import bench
    import __graft_entry__ as entry
    pkg = entry.load_package()
    ctx = bench.make_context(pkg, NCH, 8192, 0, TAPS)
    ctx.set_window(W)
    n_out = NCH + 3
    if form in TERMS:
        ctx.batch_fit_enable(fits_of(TERMS[form]))
    call, outs = ctx.batch_prepared(bench.batch_files(NCH, SR, BLOCKS), SR, "lpcm24")
    assert len(outs) == n_out
    for _ in range(3):
        call()
    ms = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()                                           # returns when every output byte is in the caller's buffers
        ms.append((time.perf_counter() - t0) * 1e3)
    kernel_us, total = -1.0, -1.0
    kib = int(ctx.get_option("stat_batch_device_kib"))
    if form in TERMS:
        rec = ctx.batch_fit()
        assert rec.shape == (N_FITS, BLOCKS) and (rec["terms"] == TERMS[form]).all()
        total = float(rec["tt"].sum())
        samples = W * 8192                               # one step of the block loop
        d_in, d_out = pkg.DeviceBuffer(ctx, NCH, samples), pkg.DeviceBuffer(ctx, 1, N_FITS * W * 46)
        d_in.upload(np.random.default_rng(1).uniform(-1.0, 1.0, (NCH, samples)))
        lists = fits_of(TERMS[form])
        for reps in (3, KERNEL_REPS):                    # warm-up, then the timed calls (each waits for its kernel)
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                ctx.block_fit_device(d_in.ptr, samples, NCH, samples, lists, d_out.ptr)
            kernel_us = (time.perf_counter() - t0) * 1e6 / reps
        d_in.free()
        d_out.free()
    ctx.close()
    print("LEG " + json.dumps({"form": form, "ms": ms, "kernel_us": kernel_us, "total": total, "kib": kib}), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    parent = os.environ.get("AB_PARENT", os.path.join(ROOT, ".ab_parent"))
    has_parent = os.path.exists(os.path.join(parent, "go-dsp-guitar_amd", "lib", "libgdg.so"))
    forms = ([("parent", parent, "off")] if has_parent else []) + [("off", ROOT, "off"), ("two", ROOT, "two"), ("eight", ROOT, "eight")]
    legs, kernels, lines = {}, {}, []
    for r in range(rounds):
        order = list(forms)
        if has_parent and r % 2:
            order[0], order[1] = order[1], order[0]
        for form, root, switches in order:
            cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", root, switches]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
            got = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
            if p.returncode != 0 or not got:
                lines.append("# %s, round %d: exit %d -- the series ends here\n%s" % (form, r + 1, p.returncode, p.stderr[-2000:]))
                report(lines, legs, kernels, forms)
                return 1
            leg = json.loads(got[0][4:])
            legs.setdefault(form, []).append(leg["ms"])
            tail = " | batch buffers %d KiB" % leg["kib"]
            if leg["kernel_us"] >= 0:
                kernels.setdefault(form, []).append(leg["kernel_us"])
                tail += " | stand-alone call, one step's rows: %.1f us | sum of tt over the records %.9g" % (leg["kernel_us"], leg["total"])
            lines.append("%-7s round %d: median %.2f | %s%s" % (form, r + 1, statistics.median(leg["ms"]), " ".join("%.2f" % v for v in leg["ms"]), tail))
            print(lines[-1], flush=True)
    report(lines, legs, kernels, forms)
    return 0


def report(lines, legs, kernels, forms):
    steps = BLOCKS // W
    head = ["# The blend fit's cost: bench.py's batch job (%d x lpcm16 x %d blocks -> lpcm24, W = %d, 2 x %d taps, %d Hz), ms of the C call." % (NCH, BLOCKS, W, TAPS, SR),
            "# Forms alternate, every leg a fresh process: 3 warm-up calls, then %d timed.  median = over all timed calls; processes = the" % CALLS,
            "# fastest .. slowest process median (the run-to-run spread); best = the fastest call.  two / eight = %d fits of 2 / 8 terms:" % N_FITS,
            "# %d records of 368 bytes per block.  off is read against parent: within the spread of the parent's processes, or the change costs something off." % N_FITS,
            "# A call has about %d steps of up to %d blocks (a quarter and a half window first, a tail of halves): per step = call / %d." % (steps + 2, W, steps)]
    if not any(f == "parent" for f, _, _ in forms):
        head.append("# NO PARENT TREE was found beside this one: the parent's legs are missing, and off has nothing to be read against.")
    for form, _, _ in forms:
        runs = legs.get(form)
        if not runs:
            continue
        allms = [v for r in runs for v in r]
        meds = [statistics.median(r) for r in runs]
        head.append("#   %-7s: median %.2f (%.3f per step)   processes %.2f .. %.2f   best %.2f   (%d processes)" % (form, statistics.median(allms), statistics.median(allms) / steps,
                                                                                                                  min(meds), max(meds), min(allms), len(runs)))
    for form, us in kernels.items():
        head.append("#   %-7s: the stand-alone call on one step's rows (%d rows x %d blocks, %d fits): median %.1f us, %.1f .. %.1f" % (form, NCH, W, N_FITS, statistics.median(us),
                                                                                                                                        min(us), max(us)))
    text = "\n".join(head + [""] + lines) + "\n"
    print(text)
    with open(os.environ.get("AB_OUT", os.path.join(ROOT, "profiles", "batch_fit_ab.txt")), "w") as f:
        f.write(text)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main())
