#!/usr/bin/env python3
"""What the dithered encoders cost a batch run: bench.py's batch job (lpcm16 files of 128 blocks -> lpcm24, W = 16, 2 x 65536 taps,
192 kHz) at 512 channels in three forms -- the parent commit, this commit with dither off, this commit with dither on -- ALTERNATING
on one machine, every leg a fresh process under its own timeout.

The parent's tree, built, is expected beside this one:
    git worktree add .ab_parent HEAD^ && make -C .ab_parent/go-dsp-guitar_amd/csrc
(AB_PARENT names another place).  Without it the parent's legs are left out and the table says so.

    python profiles/probes/batch_dither_ab.py [rounds]        -> the table on stdout (and in $AB_OUT when set)

AB_MODES=all: the parent AND this commit in each of the encoders' four modes -- plain, dithered, trimmed (every gain 0.5), trimmed with
dither -- as forms parent-off, new-off, parent-on, new-on, parent-trim, new-trim, parent-trim_on, new-trim_on (the fold of the encoders,
profiles/encode_one_path.txt).

A leg: 3 warm-up calls, then CALLS timed calls of the C call alone (arguments marshalled once, as bench.py times it); then, outside
the timed calls, 2 more calls with the encoder launches bracketed by events (profile kind K_WAVE: in a batch run without the render
report that is the encoder of every step and nothing else).  Per form the table gives the median over all timed calls of all rounds,
the fastest and slowest PROCESS median (the run-to-run spread), the fastest call, and the encoder's time per CALL -- the sum over the
call's steps, which are not all W blocks long -- with the rate at which it moves the job's bytes: (NCH + 3) rows x BLOCKS x 8192
samples x (8 read + 3 written)."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CALLS, BLOCKS, SR, TAPS, W, NCH = 9, 128, 192000, 65536, 16, 512
PROFILED = 2                                             # further calls with the encoder launches bracketed
LEG_TIMEOUT = 300                                        # seconds; a leg takes ~30 s, most of it the context's set-up
K_WAVE = 6


def child(root, form, mode=None):
    mode = mode or ("on" if form == "on" else "off")
    sys.path.insert(0, root)
    import bench
    import __graft_entry__ as entry
    pkg = entry.load_package()
    ctx = bench.make_context(pkg, NCH, 8192, 0, TAPS)
    ctx.set_window(W)
    if mode in ("on", "trim_on"):
        ctx.batch_set_dither(1, 0x5eed, 0)
    if mode in ("trim", "trim_on"):
        ctx.batch_set_trim([0.5] * NCH, 0.5, 0.5, 0.5)
    call, outs = ctx.batch_prepared(bench.batch_files(NCH, SR, BLOCKS), SR, "lpcm24")
    for _ in range(3):
        call()
    ms = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        call()                                           # returns when every output byte is in the caller's buffers
        ms.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_enable(True, kinds=[K_WAVE])
    ctx.profile_read(K_WAVE)
    for _ in range(PROFILED):
        call()
    enc_ms, enc_n = ctx.profile_read(K_WAVE)
    ctx.profile_enable(False)
    ctx.close()
    print("LEG " + json.dumps({"form": form, "ms": ms, "enc_ms": enc_ms, "enc_n": enc_n}), flush=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    parent = os.environ.get("AB_PARENT", os.path.join(ROOT, ".ab_parent"))
    forms = [("parent", parent)] if os.path.exists(os.path.join(parent, "go-dsp-guitar_amd", "lib", "libgdg.so")) else []
    forms += [("off", ROOT), ("on", ROOT)]
    modes = {"off": "off", "on": "on", "parent": "off"}
    if os.environ.get("AB_MODES") == "all":
        forms = [(who + "-" + m, root) for m in ("off", "on", "trim", "trim_on") for who, root in (("parent", parent), ("new", ROOT))]
        modes = {f: f.split("-", 1)[1] for f, _ in forms}
    legs, enc, lines = {}, {}, []
    for r in range(rounds):
        for form, root in forms:
            cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT), sys.executable, os.path.abspath(__file__), "--child", root, form, modes[form]]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=root)
            got = [l for l in p.stdout.splitlines() if l.startswith("LEG ")]
            if p.returncode != 0 or not got:
                lines.append("# %s, round %d: exit %d -- the series ends here\n%s" % (form, r + 1, p.returncode, p.stderr[-2000:]))
                report(lines, legs, enc, forms)
                return 1
            leg = json.loads(got[0][4:])
            legs.setdefault(form, []).append(leg["ms"])
            if leg["enc_n"]:
                enc.setdefault(form, []).append(leg["enc_ms"] / PROFILED)
            lines.append("%-14s round %d: median %.2f | %s | encoder %.3f ms per call (%d launches in %d calls)" % (
                form, r + 1, statistics.median(leg["ms"]), " ".join("%.2f" % v for v in leg["ms"]), leg["enc_ms"] / PROFILED, leg["enc_n"], PROFILED))
            print(lines[-1], flush=True)
    report(lines, legs, enc, forms)
    return 0


def report(lines, legs, enc, forms):
    call_bytes = (NCH + 3) * BLOCKS * 8192 * (8 + 3)         # every output sample of the job: 8 bytes read and 3 written
    head = ["# The dithered encoders' cost: bench.py's batch job (%d channels, lpcm16 x %d blocks -> lpcm24, W = %d, 2 x %d taps, %d Hz), ms of the C call." % (
                NCH, BLOCKS, W, TAPS, SR),
            "# Forms alternate, every leg a fresh process: 3 warm-up calls, then %d timed.  median = over all timed calls; processes = the" % CALLS,
            "# fastest .. slowest process median (the run-to-run spread); best = the fastest call.  encoder = the encode launches of one call,",
            "# summed, bracketed by events in %d further calls; its rate = the job's %.1f MB (%d rows x %d blocks x 8192 samples x 11 bytes) over that time." % (
                PROFILED, call_bytes / 1e6, NCH + 3, BLOCKS)]
    if not any(f.startswith("parent") for f, _ in forms):
        head.append("# NO PARENT TREE was found beside this one: the parent's legs are missing.")
    for form, _ in forms:
        runs = legs.get(form)
        if not runs:
            continue
        allms = [v for r in runs for v in r]
        meds = [statistics.median(r) for r in runs]
        e = enc.get(form, [])
        tail = "   encoder %.3f ms per call (%.3f .. %.3f), %.2f TB/s" % (statistics.median(e), min(e), max(e), call_bytes / (statistics.median(e) * 1e-3) / 1e12) if e else ""
        head.append("#   %-14s: median %.2f   processes %.2f .. %.2f   best %.2f   (%d processes)%s" % (form, statistics.median(allms), min(meds), max(meds), min(allms),
                                                                                                  len(runs), tail))
    if legs.get("on") and legs.get("off"):
        on, off = statistics.median([v for r in legs["on"] for v in r]), statistics.median([v for r in legs["off"] for v in r])
        head.append("#   on / off, the whole call: %.4f" % (on / off))
        if enc.get("on") and enc.get("off"):
            head.append("#   on / off, the encoder:    %.3f" % (statistics.median(enc["on"]) / statistics.median(enc["off"])))
    if legs.get("parent") and legs.get("off"):
        par, off = statistics.median([v for r in legs["parent"] for v in r]), statistics.median([v for r in legs["off"] for v in r])
        head.append("#   off / parent, the whole call: %.4f" % (off / par))
    text = "\n".join(head + [""] + lines) + "\n"
    print(text)
    if os.environ.get("AB_OUT"):
        with open(os.environ["AB_OUT"], "w") as f:
            f.write(text)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:5])
    else:
        sys.exit(main())
