#!/usr/bin/env python3
"""What the true-peak records cost a batch run: bench.py's batch job (512 lpcm16 files of 128 blocks -> lpcm24, W = 16, 2 x 65536 taps,
192 kHz) in three forms -- the parent commit, this commit with the switch off, this commit with the switch on (all N + 3
ports) -- ALTERNATING on one machine, every leg a fresh process under its own timeout.

The parent's tree, built, is expected beside this one:
    git worktree add .ab_parent HEAD^ && make -C .ab_parent/go-dsp-guitar_amd/csrc
(AB_PARENT names another place).  Without it the parent's legs are left out and the table says so.

    python profiles/probes/batch_true_peak_ab.py [rounds]         -> the table on stdout and in profiles/batch_true_peak_ab.txt ($AB_OUT: elsewhere)
    python profiles/probes/batch_true_peak_ab.py [rounds] off,four

The second form names the legs itself, for a change that must not move the block loop's host side: "four" = all four kinds of the render
report on (statistics, ten octave bands, every chain port aligned against port 0, true peak), and the parent runs every named leg too
(as "parent" for off, "parent-four" for four; a parent that has no true-peak switch cannot run on or four).  Rounds alternate which of
a pair runs first.

A leg: 3 warm-up calls, then CALLS timed calls of the C call alone (arguments marshalled once, as bench.py times it).  Per form the
table gives the median over all timed calls of all rounds, the fastest and slowest PROCESS median (the run-to-run spread) and the
fastest call.  The "on" legs also time the kernel alone on a buffer of a step's shape -- 515 rows of 16 blocks, the stand-alone
device entry, KERNEL_REPS calls between two synchronisations -- which is the kernel's time per step of the block loop."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CALLS, BLOCKS, SR, TAPS, W, NCH = 9, 128, 192000, 65536, 16, 512
KERNEL_REPS = 20
EDGES = [31.25 * 2.0 ** i for i in range(11)]            # "four": ten octave bands, 31.25 Hz .. 32 kHz (batch_spectrum_ab.py's)
REFS, MAX_LAG = [0] * NCH + [-1, -1, -1], 2048           # ... every chain port against port 0 (batch_align_ab.py's)
LEG_TIMEOUT = 300                                        # seconds; a leg takes ~20 s, most of it the context's set-up


def child(root, form):
    sys.path.insert(0, root)
    import numpy as np
    import bench
    import __graft_entry__ as entry
    pkg = entry.load_package()
    ctx = bench.make_context(pkg, NCH, 8192, 0, TAPS)
    ctx.set_window(W)
    if form in ("on", "four"):
        ctx.batch_true_peak_enable()
    if form == "four":
        ctx.batch_report_enable()
        ctx.batch_spectrum_enable(EDGES)
        ctx.batch_align_enable(REFS, MAX_LAG)
    call, outs = ctx.batch_prepared(bench.batch_files(NCH, SR, BLOCKS), SR, "lpcm24")
    for _ in range(3):
        call()
    ms = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()                                           # returns when every output byte is in the caller's buffers
        ms.append((time.perf_counter() - t0) * 1e3)
    kernel_us, total = -1.0, -1.0
    if form in ("on", "four"):
        rec = ctx.batch_true_peak()
        assert rec.shape == (NCH + 3, BLOCKS)
        total = float(rec["true_peak"].sum())
    if form == "four":
        assert ctx.batch_report().shape == (NCH + 3, BLOCKS) and ctx.batch_spectrum().shape == (NCH + 3, BLOCKS, len(EDGES) - 1) and ctx.batch_align().shape == (NCH + 3, BLOCKS)
    if form == "on":
        rows, samples = NCH + 3, W * 8192                # one step of the block loop
        d_in, d_out = pkg.DeviceBuffer(ctx, rows, samples), pkg.DeviceBuffer(ctx, rows, W * 2)
        d_in.upload(np.random.default_rng(1).uniform(-1.0, 1.0, (rows, samples)))
        for reps in (3, KERNEL_REPS):                    # warm-up, then the timed launches
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                ctx.block_true_peak_device(d_in.ptr, samples, rows, samples, d_out.ptr)
            ctx.synchronize()
            kernel_us = (time.perf_counter() - t0) * 1e6 / reps
        d_in.free()
        d_out.free()
    ctx.close()
    print("LEG " + json.dumps({"form": form, "ms": ms, "kernel_us": kernel_us, "total": total}), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    parent = os.environ.get("AB_PARENT", os.path.join(ROOT, ".ab_parent"))
    has_parent = os.path.exists(os.path.join(parent, "go-dsp-guitar_amd", "lib", "libgdg.so"))
    named = sys.argv[2].split(",") if len(sys.argv) > 2 else None
    if named:                                            # every named leg on the parent's tree and on this one
        forms = [("parent" if f == "off" else "parent-" + f, parent, f) for f in named if has_parent] + [(f, ROOT, f) for f in named]
        forms.sort(key=lambda t: named.index(t[2]))      # parent, off, parent-four, four: a leg next to its counterpart
    else:
        forms = ([("parent", parent, "off")] if has_parent else []) + [("off", ROOT, "off"), ("on", ROOT, "on")]
    legs, kernels, lines = {}, [], []
    for r in range(rounds):
        order = forms
        if named and has_parent and r % 2:               # odd rounds: this tree's leg in front of its parent's, so that neither always runs second
            order = [forms[i ^ 1] for i in range(len(forms))]
        for form, root, switches in order:
            cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", root, switches]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
            got = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
            if p.returncode != 0 or not got:
                lines.append("# %s, round %d: exit %d -- the series ends here\n%s" % (form, r + 1, p.returncode, p.stderr[-2000:]))
                report(lines, legs, kernels, forms)
                return 1
            leg = json.loads(got[0][4:])
            leg["form"] = form
            legs.setdefault(form, []).append(leg["ms"])
            tail = ""
            if leg["kernel_us"] >= 0:
                kernels.append(leg["kernel_us"])
                tail = " | kernel alone, one step's rows: %.1f us | sum of true_peak %.9g" % (leg["kernel_us"], leg["total"])
            elif leg["total"] >= 0:
                tail = " | sum of true_peak %.9g" % leg["total"]
            lines.append("%-11s round %d: median %.2f | %s%s" % (form, r + 1, statistics.median(leg["ms"]), " ".join("%.2f" % v for v in leg["ms"]), tail))
            print(lines[-1], flush=True)
    report(lines, legs, kernels, forms)
    return 0


def report(lines, legs, kernels, forms):
    steps = BLOCKS // W
    title = "Parent against this tree, leg by leg" if any(f.startswith("parent-") for f, _, _ in forms) else "The true-peak records' cost"
    head = ["# %s: bench.py's batch job (%d x lpcm16 x %d blocks -> lpcm24, W = %d, 2 x %d taps, %d Hz), ms of the C call." % (title, NCH, BLOCKS, W, TAPS, SR),
            "# Forms alternate, every leg a fresh process: 3 warm-up calls, then %d timed.  median = over all timed calls; processes = the" % CALLS,
            "# fastest .. slowest process median (the run-to-run spread); best = the fastest call.  on = all %d ports; four = all four" % (NCH + 3),
            "# kinds of the render report on (statistics, %d bands, %d ports aligned against port 0, true peak)." % (len(EDGES) - 1, NCH),
            "# A call has about %d steps of up to %d blocks (a quarter and a half window first, a tail of halves): per step = call / %d." % (steps + 2, W, steps)]
    if not any(f == "parent" for f, _, _ in forms):
        head.append("# NO PARENT TREE was found beside this one: the parent's legs are missing.")
    for form, _, _ in forms:
        runs = legs.get(form)
        if not runs:
            continue
        allms = [v for r in runs for v in r]
        meds = [statistics.median(r) for r in runs]
        head.append("#   %-11s: median %.2f (%.3f per step)   processes %.2f .. %.2f   best %.2f   (%d processes)" % (form, statistics.median(allms), statistics.median(allms) / steps,
                                                                                                                   min(meds), max(meds), min(allms), len(runs)))
    if kernels:
        head.append("#   the kernel alone on one step's rows (%d rows x %d blocks): median %.1f us, %.1f .. %.1f" % (NCH + 3, W, statistics.median(kernels), min(kernels), max(kernels)))
    text = "\n".join(head + [""] + lines) + "\n"
    print(text)
    with open(os.environ.get("AB_OUT", os.path.join(ROOT, "profiles", "batch_true_peak_ab.txt")), "w") as f:
        f.write(text)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main())
