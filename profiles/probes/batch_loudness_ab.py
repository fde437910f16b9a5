#!/usr/bin/env python3
"""What the loudness records cost a batch run: bench.py's batch job (512 lpcm16 files of 128 blocks -> lpcm24, W = 16, 2 x 65536 taps,
192 kHz) in three forms -- the parent commit, this commit with the records never enabled, and enabled -- ALTERNATING on one machine, every
leg a fresh process under its own timeout.

The parent's tree, built, is expected beside this one:
    git worktree add .ab_parent HEAD^ && make -C .ab_parent/go-dsp-guitar_amd/csrc
(AB_PARENT names another place).  Without it the parent's legs are left out and the table says so.  The never-set leg is to be read against
the parent's, never against itself, and it must report the parent's stat_batch_device_kib and output bytes (a checksum of the last call's
outputs is printed for every leg).

    python profiles/probes/batch_loudness_ab.py [rounds]   -> the table on stdout and in profiles/batch_loudness_ab.txt ($AB_OUT: elsewhere)

Odd rounds run "never" in front of "parent", so that neither always runs second.  A leg: 3 warm-up calls, then CALLS timed calls of the C
call alone (arguments marshalled once, as bench.py times it).  Per form the table gives the median over all timed calls of all rounds, the
fastest and slowest PROCESS median (the run-to-run spread), the median of the processes' fastest calls and the fastest call.  The
enabled leg also times the stand-alone device entry on one step's rows -- 515 rows of 16 blocks, the state carried; the legs synchronise
around it: an upper bound of the kernel's time per step -- and every leg prints the bytes a call writes."""
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CALLS, BLOCKS, SR, TAPS, W, NCH = 9, 128, 192000, 65536, 16, 512
KERNEL_REPS = 20
LEG_TIMEOUT = 300                                        # seconds; a leg takes ~20 s, most of it the context's set-up
FORMS = ("on",)                                          # the legs with the records on


def child(root, form):
    sys.path.insert(0, root)
    import numpy as np
    import bench
    import __graft_entry__ as entry
    pkg = entry.load_package()
    ctx = bench.make_context(pkg, NCH, 8192, 0, TAPS)
    ctx.set_window(W)
    n_out = NCH + 3
    if form in FORMS:
        ctx.batch_loudness_enable()
    call, outs = ctx.batch_prepared(bench.batch_files(NCH, SR, BLOCKS), SR, "lpcm24")
    assert len(outs) == n_out and outs[0].size == BLOCKS * 8192 * 3
    for _ in range(3):
        call()
    ms = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()                                           # returns when every output byte is in the caller's buffers
        ms.append((time.perf_counter() - t0) * 1e3)
    crc = 0
    for o in outs[:NCH + 3]:
        crc = zlib.crc32(memoryview(np.ascontiguousarray(o)).cast("B"), crc)
    kernel_us, total = [], float(sum(o.size for o in outs))
    kib = int(ctx.get_option("stat_batch_device_kib"))
    if form in FORMS:
        assert ctx.batch_loudness().shape == (n_out, pkg.loudness_hops(SR, 0, BLOCKS * 8192))
        samples = W * 8192                               # one step of the block loop: W blocks of every row
        hops = pkg.loudness_hops(SR, 0, samples)
        d_in, d_out, d_hist = pkg.DeviceBuffer(ctx, n_out, samples), pkg.DeviceBuffer(ctx, n_out, hops), pkg.DeviceBuffer(ctx, n_out, pkg.LOUDNESS_STATE_DOUBLES)
        d_in.upload(np.random.default_rng(1).uniform(-1.0, 1.0, (n_out, samples)))
        for reps in (3, KERNEL_REPS):                    # warm-up, then the timed calls
            kernel_us = []
            for _ in range(reps):
                ctx.synchronize()
                t0 = time.perf_counter()
                ctx.loudness_rows_device(d_in.ptr, samples, n_out, 0, samples, SR, None, d_hist.ptr, d_out.ptr, hops)
                ctx.synchronize()
                kernel_us.append((time.perf_counter() - t0) * 1e6)
        for b in (d_in, d_out, d_hist):
            b.free()
    ctx.close()
    print("LEG " + json.dumps({"form": form, "ms": ms, "kernel_us": kernel_us, "total": total, "kib": kib, "crc": crc}), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    parent = os.environ.get("AB_PARENT", os.path.join(ROOT, ".ab_parent"))
    has_parent = os.path.exists(os.path.join(parent, "go-dsp-guitar_amd", "lib", "libgdg.so"))
    forms = ([("parent", parent, "never")] if has_parent else []) + [("never", ROOT, "never"), ("on", ROOT, "on")]
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
            line = "%-7s round %d: median %.2f | %s | batch buffers %d KiB | outputs crc %08x" % (form, r + 1, statistics.median(leg["ms"]), " ".join("%.2f" % v for v in leg["ms"]),
                                                                                                  leg["kib"], leg["crc"])
            line += " | %.1f MB written" % (leg["total"] / 1e6)
            if leg["kernel_us"]:
                kernels.setdefault(form, []).extend(leg["kernel_us"])
                line += " | stand-alone call, one step's rows: median %.1f us" % statistics.median(leg["kernel_us"])
            lines.append(line)
            print(line, flush=True)
    steps = BLOCKS // W
    head = ["# The cost of the loudness records: bench.py's batch job (%d x lpcm16 x %d blocks -> lpcm24, W = %d, 2 x %d taps, %d Hz), ms of the C call." % (NCH, BLOCKS, W, TAPS, SR),
            "# Forms alternate, every leg a fresh process: 3 warm-up calls, then %d timed.  median = over all timed calls; processes = the" % CALLS,
            "# fastest .. slowest process median (the run-to-run spread); fastest = the median of the processes' fastest calls; best = the fastest call.",
            "# parent, never = no records.  on = the same job with gdg_batch_loudness_enable.",
            "# never is read against parent: within the spread of the parent's processes, or the change costs something off.  on is read against parent too.",
            "# No figure is fixed in advance for on: one launch more per step, one workgroup per port, nothing more on the way down.",
            "# A call has about %d steps of up to %d blocks (a quarter and a half window first, a tail of halves): per step = call / %d." % (steps + 2, W, steps)]
    if not any(f == "parent" for f, _, _ in forms):
        head.append("# NO PARENT TREE was found beside this one: the parent's legs are missing, and never has nothing to be read against.")
    for form, _, _ in forms:
        runs = legs.get(form)
        if not runs:
            continue
        allms = [v for r in runs for v in r]
        meds = [statistics.median(r) for r in runs]
        head.append("#   %-7s: median %.2f (%.3f per step)   processes %.2f .. %.2f   fastest %.2f   best %.2f   (%d processes)" % (
            form, statistics.median(allms), statistics.median(allms) / steps, min(meds), max(meds), statistics.median([min(r) for r in runs]), min(allms), len(runs)))
    for form, us in kernels.items():
        med, best = statistics.median(us), min(us)
        head.append("#   %-7s: gdg_loudness_rows_device on one step's rows (%d rows x %d blocks, the state zeroed and carried): median %.1f us, %.1f .. %.1f "
                    "(measured between two waits for the stream: an upper bound)" % (form, NCH + 3, W, med, best, max(us)))
    text = "\n".join(head + [""] + lines) + "\n"
    print(text)
    with open(os.environ.get("AB_OUT", os.path.join(ROOT, "profiles", "batch_loudness_ab.txt")), "w") as f:
        f.write(text)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main())
