#!/usr/bin/env python3
"""What the Gram records cost a batch run: bench.py's batch job (512 lpcm16 files of 128 blocks -> lpcm24, W = 16, 2 x 65536 taps,
192 kHz) in four forms -- the parent commit, this commit with the list off, with a list of 64 ports and with a list of 512 ports --
ALTERNATING on one machine, every leg a fresh process under its own timeout.

The parent's tree, built, is expected beside this one:
    git worktree add .ab_parent HEAD^ && make -C .ab_parent/go-dsp-guitar_amd/csrc
(AB_PARENT names another place).  Without it the parent's legs are left out and the table says so.  The off leg is to be read against the
parent's, never against itself: it may differ from the parent's median by the spread of the parent's own process medians and no more.

    python profiles/probes/batch_gram.py [rounds]          -> the table on stdout and in profiles/batch_gram_ab.txt ($AB_OUT: elsewhere)

Odd rounds run "off" in front of "parent", so that neither always runs second.  A leg: 3 warm-up calls, then CALLS timed calls of the C
call alone (arguments marshalled once, as bench.py times it).  Per form the table gives the median over all timed calls of all rounds, the
fastest and slowest PROCESS median (the run-to-run spread) and the fastest call.  The list legs also time the stand-alone device entry on
512 rows of 16 blocks -- one step of the block loop; the entry uploads its list and waits, so the figure is an upper bound of the
kernel's time per step -- and report what it achieved: FLOP/s counting 2 L per entry of the lower triangle, tiles' zero padding not
counted, and the bytes the workgroups read (two 64-row panels per tile, one for a diagonal tile), most of them cache hits.  The trace of
the last call's summed Gram is printed, so that a leg that measured nothing shows."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CALLS, BLOCKS, SR, TAPS, W, NCH = 9, 128, 192000, 65536, 16, 512
KERNEL_REPS = 20
LEG_TIMEOUT = 300                                        # seconds; a leg takes ~20 s, most of it the context's set-up
PORTS = {"p64": 64, "p512": 512}


def list_of(n):
    """n different ports spread over the job's channels"""
    return [(k * (NCH // n) + 3) % NCH for k in range(n)]


def child(root, form):
    sys.path.insert(0, root)
    import numpy as np
    import bench
    import __graft_entry__ as entry
    pkg = entry.load_package()
    ctx = bench.make_context(pkg, NCH, 8192, 0, TAPS)
    ctx.set_window(W)
    n_out = NCH + 3
    if form in PORTS:
        ctx.batch_gram_enable(list_of(PORTS[form]))
    call, outs = ctx.batch_prepared(bench.batch_files(NCH, SR, BLOCKS), SR, "lpcm24")
    assert len(outs) == n_out
    for _ in range(3):
        call()
    ms = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()                                           # returns when every output byte is in the caller's buffers
        ms.append((time.perf_counter() - t0) * 1e3)
    kernel_us, total = [], -1.0
    kib = int(ctx.get_option("stat_batch_device_kib"))
    if form in PORTS:
        P = PORTS[form]
        rec = ctx.batch_gram()
        assert rec.shape == (BLOCKS, P * (P + 1) // 2)
        diag = [i * (i + 1) // 2 + i for i in range(P)]
        total = float(rec[:, diag].sum())
        samples = W * 8192                               # one step of the block loop
        d_in, d_out = pkg.DeviceBuffer(ctx, NCH, samples), pkg.DeviceBuffer(ctx, 1, W * (P * (P + 1) // 2))
        d_in.upload(np.random.default_rng(1).uniform(-1.0, 1.0, (NCH, samples)))
        ports = list_of(P)
        for reps in (3, KERNEL_REPS):                    # warm-up, then the timed calls (each waits for its kernel)
            ctx.synchronize()
            kernel_us = []
            for _ in range(reps):
                t0 = time.perf_counter()
                ctx.block_gram_device(d_in.ptr, samples, NCH, samples, ports, d_out.ptr)
                kernel_us.append((time.perf_counter() - t0) * 1e6)
        d_in.free()
        d_out.free()
    ctx.close()
    print("LEG " + json.dumps({"form": form, "ms": ms, "kernel_us": kernel_us, "total": total, "kib": kib}), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    parent = os.environ.get("AB_PARENT", os.path.join(ROOT, ".ab_parent"))
    has_parent = os.path.exists(os.path.join(parent, "go-dsp-guitar_amd", "lib", "libgdg.so"))
    forms = ([("parent", parent, "off")] if has_parent else []) + [("off", ROOT, "off"), ("p64", ROOT, "p64"), ("p512", ROOT, "p512")]
    legs, kernels, lines = {}, {}, []
    for r in range(rounds):
        order = list(forms)
        if has_parent and r % 2:
            order[0], order[1] = order[1], order[0]
        for form, root, switches in order:
            cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", root, switches]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
            got = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
            if p.returncode != 0 or not got:             # a leg that died: nothing more is started on the device
                print("leg %s of round %d ended with status %d\n%s\n%s" % (form, r + 1, p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
                return 1
            leg = json.loads(got[-1][4:])
            legs.setdefault(form, []).append(leg["ms"])
            line = "%-7s round %d: median %.2f | %s | batch buffers %d KiB" % (form, r + 1, statistics.median(leg["ms"]), " ".join("%.2f" % v for v in leg["ms"]), leg["kib"])
            if leg["kernel_us"]:
                kernels.setdefault(form, []).extend(leg["kernel_us"])
                line += " | stand-alone call, one step's rows: median %.1f us | trace of the summed Gram %.3f" % (statistics.median(leg["kernel_us"]), leg["total"])
            lines.append(line)
            print(line, flush=True)
    steps = BLOCKS // W
    head = ["# The Gram records' cost: bench.py's batch job (%d x lpcm16 x %d blocks -> lpcm24, W = %d, 2 x %d taps, %d Hz), ms of the C call." % (NCH, BLOCKS, W, TAPS, SR),
            "# Forms alternate, every leg a fresh process: 3 warm-up calls, then %d timed.  median = over all timed calls; processes = the" % CALLS,
            "# fastest .. slowest process median (the run-to-run spread); best = the fastest call.  p64 / p512 = a list of 64 / 512 ports:",
            "# one record of 16 640 / 1 050 624 bytes per block.  off is read against parent: within the spread of the parent's processes, or the change costs something off.",
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
        P = PORTS[form]
        T = -(-P // 64)
        flop = 2.0 * 8192 * (P * (P + 1) // 2) * W
        read = W * 8192 * 8.0 * 64 * (T * (T + 1) // 2 * 2 - T)
        med, best = statistics.median(us), min(us)
        head.append("#   %-7s: the stand-alone call on one step's rows (%d rows x %d blocks, P = %d): median %.1f us, %.1f .. %.1f; %.3g FLOP and %.3g bytes read by the workgroups: "
                    "%.2f TFLOP/s and %.2f TB/s at the median, %.2f TFLOP/s at the fastest call (measured; upload of the list and the wait included)" % (
                        form, NCH, W, P, med, best, max(us), flop, read, flop / med * 1e-6, read / med * 1e-6, flop / best * 1e-6))
    text = "\n".join(head + [""] + lines) + "\n"
    print(text)
    with open(os.environ.get("AB_OUT", os.path.join(ROOT, "profiles", "batch_gram_ab.txt")), "w") as f:
        f.write(text)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main())
