#!/usr/bin/env python3
"""What a short FIR per blend term costs a batch run: bench.py's batch job (512 lpcm16 files of 128 blocks -> lpcm24, W = 16, 2 x 65536
taps, 192 kHz) with 64 two-term blends in three forms -- the parent commit, this commit with the same blends and no taps (which must run
the parent's launches), this commit with the same blends and 32 taps on every second term -- ALTERNATING on one machine, every leg a fresh
process under its own timeout.

The parent's tree, built, is expected beside this one:
    git worktree add .ab_parent HEAD^ && make -C .ab_parent/go-dsp-guitar_amd/csrc
(AB_PARENT names another place).  Without it the parent's legs are left out and the table says so.  The off leg is to be read against the
parent's, never against itself: it may differ from the parent's median by the spread of the parent's own process medians and no more.

    python profiles/probes/batch_blend_filter.py [rounds]   -> the table on stdout and in profiles/batch_blend_filter_ab.txt ($AB_OUT: elsewhere)

Odd rounds run "off" in front of "parent", so that neither always runs second.  A leg: 3 warm-up calls, then CALLS timed calls of the C
call alone (arguments marshalled once, as bench.py times it).  Per form the table gives the median over all timed calls of all rounds, the
fastest and slowest PROCESS median (the run-to-run spread) and the fastest call; every leg prints its batch buffers' size (the taps
leg's holds the history, 512 x 4096 doubles = 16 MiB) and the sum of the first bytes of the last blend file, so that a leg that wrote
nothing -- or a off leg that wrote something else than the parent -- shows."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CALLS, BLOCKS, SR, TAPS, W, NCH = 9, 128, 192000, 65536, 16, 512
N_BLENDS = 64
LEG_TIMEOUT = 300                                        # seconds; a leg takes ~20 s, most of it the context's set-up


def blends_of(taps, pkg):
    """blend b: two channels spread over the job at 0.5 and -1.0; taps: the second term through 32 windowed-sinc taps for a fraction of (b mod 4) / 4"""
    out = []
    for b in range(N_BLENDS):
        terms = [((b * 8 + k * 61) % NCH, (1.0 + k) / 2 * (-1.0 if k & 1 else 1.0)) for k in range(2)]
        if taps:
            terms = [terms[0] + (0, []), terms[1] + (0, pkg.blend_fraction_taps(32, (b % 4) / 4.0))]
        out.append(terms)
    return out


def child(root, form):
    sys.path.insert(0, root)
    import numpy as np
    import bench
    import __graft_entry__ as entry
    pkg = entry.load_package()
    ctx = bench.make_context(pkg, NCH, 8192, 0, TAPS)
    ctx.set_window(W)
    ctx.batch_set_blends(blends_of(form == "taps", pkg))
    call, outs = ctx.batch_prepared(bench.batch_files(NCH, SR, BLOCKS), SR, "lpcm24")
    assert len(outs) == NCH + 3 + N_BLENDS
    for _ in range(3):
        call()
    ms = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()                                           # returns when every output byte is in the caller's buffers
        ms.append((time.perf_counter() - t0) * 1e3)
    kib = int(ctx.get_option("stat_batch_device_kib"))
    total = float(outs[-1][:3 * 8192].astype(np.float64).sum())
    ctx.close()
    print("LEG " + json.dumps({"form": form, "ms": ms, "total": total, "kib": kib}), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    parent = os.environ.get("AB_PARENT", os.path.join(ROOT, ".ab_parent"))
    has_parent = os.path.exists(os.path.join(parent, "go-dsp-guitar_amd", "lib", "libgdg.so"))
    forms = ([("parent", parent, "off")] if has_parent else []) + [("off", ROOT, "off"), ("taps", ROOT, "taps")]
    legs, lines = {}, []
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
                report(lines, legs, forms)
                return 1
            leg = json.loads(got[0][4:])
            legs.setdefault(form, []).append(leg["ms"])
            lines.append("%-7s round %d: median %.2f | %s | batch buffers %d KiB | last blend file, first bytes' sum %.9g" % (
                form, r + 1, statistics.median(leg["ms"]), " ".join("%.2f" % v for v in leg["ms"]), leg["kib"], leg["total"]))
            print(lines[-1], flush=True)
    report(lines, legs, forms)
    return 0


def report(lines, legs, forms):
    steps = BLOCKS // W
    head = ["# A short FIR per blend term: bench.py's batch job (%d x lpcm16 x %d blocks -> lpcm24, W = %d, 2 x %d taps, %d Hz) with %d two-term blends," % (NCH, BLOCKS, W, TAPS, SR, N_BLENDS),
            "# ms of the C call.  Forms alternate, every leg a fresh process: 3 warm-up calls, then %d timed.  median = over all timed calls;" % CALLS,
            "# processes = the fastest .. slowest process median (the run-to-run spread); best = the fastest call.  off = no taps: the parent's",
            "# launches, read against parent.  taps = the second term of every blend through 32 windowed-sinc taps: the filtered kernel and the",
            "# history save per step.  A call has about %d steps: per step = call / %d." % (steps + 2, steps)]
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
    text = "\n".join(head + [""] + lines) + "\n"
    print(text)
    with open(os.environ.get("AB_OUT", os.path.join(ROOT, "profiles", "batch_blend_filter_ab.txt")), "w") as f:
        f.write(text)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
    else:
        sys.exit(main())
