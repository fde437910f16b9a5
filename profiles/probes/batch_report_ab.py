#!/usr/bin/env python3
"""What the render report costs a batch run: bench.py's batch job (lpcm16 files of 128 blocks -> lpcm24, W = 16, 2 x 65536 taps, 192 kHz)
at 64 and 512 channels in three forms -- the parent commit, this commit with the report off, this commit with the report on --
ALTERNATING on one machine, every leg a fresh process under its own timeout.

The parent's tree, built, is expected beside this one:
    git worktree add .ab_parent HEAD^ && make -C .ab_parent/go-dsp-guitar_amd/csrc
(AB_PARENT names another place).  Without it the parent's legs are left out and the table says so.

    python profiles/probes/batch_report_ab.py [rounds]        -> the table on stdout (and in $AB_OUT when set)

A leg: 3 warm-up calls, then CALLS timed calls of the C call alone (arguments marshalled once, as bench.py times it).  Per form and
channel count the table gives the median over all timed calls of all rounds, the fastest and slowest PROCESS median (the run-to-run
spread) and the fastest call."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CALLS, BLOCKS, SR, TAPS, W = 9, 128, 192000, 65536, 16
LEG_TIMEOUT = 240                                        # seconds; a leg takes ~20 s, most of it the context's set-up


def child(root, form, nch):
    sys.path.insert(0, root)
    import bench
    import __graft_entry__ as entry
    pkg = entry.load_package()
    ctx = bench.make_context(pkg, nch, 8192, 0, TAPS)
    ctx.set_window(W)
    if form == "on":
        ctx.batch_report_enable(True)
    call, outs = ctx.batch_prepared(bench.batch_files(nch, SR, BLOCKS), SR, "lpcm24")
    for _ in range(3):
        call()
    ms = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()                                           # returns when every output byte is in the caller's buffers
        ms.append((time.perf_counter() - t0) * 1e3)
    clipped = int(ctx.batch_report()["clipped"].astype("u8").sum()) if form == "on" else -1
    ctx.close()
    print("LEG " + json.dumps({"form": form, "nch": nch, "ms": ms, "clipped": clipped}), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    parent = os.environ.get("AB_PARENT", os.path.join(ROOT, ".ab_parent"))
    forms = [("parent", parent)] if os.path.exists(os.path.join(parent, "go-dsp-guitar_amd", "lib", "libgdg.so")) else []
    forms += [("off", ROOT), ("on", ROOT)]
    legs = {}
    lines = []
    for nch in (64, 512):
        for r in range(rounds):
            for form, root in forms:
                cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", root, form, str(nch)]
                p = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
                got = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
                if p.returncode != 0 or not got:
                    lines.append("# %s, %d channels, round %d: exit %d -- the series ends here\n%s" % (form, nch, r + 1, p.returncode, p.stderr[-2000:]))
                    report(lines, legs, forms)
                    return 1
                leg = json.loads(got[0][4:])
                legs.setdefault((form, nch), []).append(leg["ms"])
                lines.append("%-6s %3d ch round %d: median %.2f | %s%s" % (form, nch, r + 1, statistics.median(leg["ms"]), " ".join("%.2f" % v for v in leg["ms"]),
                                                                             "" if leg["clipped"] < 0 else " | clipped samples reported: %d" % leg["clipped"]))
                print(lines[-1], flush=True)
    report(lines, legs, forms)
    return 0


def report(lines, legs, forms):
    head = ["# The render report's cost: bench.py's batch job (lpcm16 x %d blocks -> lpcm24, W = %d, 2 x %d taps, %d Hz), ms of the C call." % (BLOCKS, W, TAPS, SR),
            "# Forms alternate, every leg a fresh process: 3 warm-up calls, then %d timed.  median = over all timed calls; processes = the" % CALLS,
            "# fastest .. slowest process median (the run-to-run spread); best = the fastest call.",
            "# Traffic: the report reads 8 bytes per output sample once more, beside the 608 bytes per sample VERDICT.md counts for this chain: +1.3 %."]
    if not any(f == "parent" for f, _ in forms):
        head.append("# NO PARENT TREE was found beside this one: the parent's legs are missing.")
    for nch in (64, 512):
        for form, _ in forms:
            runs = legs.get((form, nch))
            if not runs:
                continue
            allms = [v for r in runs for v in r]
            meds = [statistics.median(r) for r in runs]
            head.append("#   %3d channels, %-6s: median %.2f   processes %.2f .. %.2f   best %.2f   (%d processes)" % (nch, form, statistics.median(allms), min(meds), max(meds),
                                                                                                                      min(allms), len(runs)))
    text = "\n".join(head + [""] + lines) + "\n"
    print(text)
    if os.environ.get("AB_OUT"):
        with open(os.environ["AB_OUT"], "w") as f:
            f.write(text)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        sys.exit(main())
