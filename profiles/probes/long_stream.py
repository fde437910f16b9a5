#!/usr/bin/env python3
"""Where on the parity gate's stream does the device leave the oracle?  ("What's weak", first bullet.)

The localiser behind tests/test_gpu_long_stream.py: global channels 0 / 256 / 511 of the bench's job on one-channel contexts, 176 calls
round robin over bench.synth_blocks' 4 blocks, compared with the oracle per block -- the full chain at the bench's 65536 taps, then every
prefix of bench.CHAIN and every unit alone on the oracle's intermediate signal at --taps; then the driver's control-call sequence against
plain calls, and windows of 16 against per-frame calls, bit for bit.

    python profiles/probes/long_stream.py [--taps 8192] [--channels 0,256,511] > profiles/parity_long_stream.txt
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import bench  # noqa: E402
import test_long_stream_host as ls  # noqa: E402
import test_gpu_long_stream as gl  # noqa: E402

LOUD = 1e-12          # a block is listed when its RMS distance is above this (the quiet stream sits at 1e-16 .. 1e-14)


def runs(idx):
    """[3, 4, 5, 9] -> '3-5, 9'"""
    out, i = [], 0
    while i < len(idx):
        j = i
        while j + 1 < len(idx) and idx[j + 1] == idx[j] + 1:
            j += 1
        out.append("%d" % idx[i] if i == j else "%d-%d" % (idx[i], idx[j]))
        i = j + 1
    return ", ".join(out) if out else "none"


def row(label, rms, mx, limit=None):
    w = int(rms.argmax())
    loud = [int(b) for b in np.nonzero(rms > LOUD)[0]]
    s = "%-34s worst block %3d  rms %.3e  max_abs %.3e  median %.3e" % (label, w, rms[w], mx[w], float(np.median(rms)))
    if limit is not None:
        s += "  bound %.3e  ratio %7.3f" % (limit, rms[w] / limit)
    s += "  blocks > %.0e: %s" % (LOUD, runs(loud))
    print(s, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--taps", type=int, default=ls.TAPS, help="IR length of the prefix and unit tables")
    ap.add_argument("--channels", default=",".join(str(g) for g in ls.CHANNELS))
    ap.add_argument("--no-repro", action="store_true", help="skip the 65536-tap reproduction")
    args = ap.parse_args()
    channels = [int(g) for g in args.channels.split(",")]
    pkg = entry.load_package()
    orc = entry.load_oracle()
    orc.build()

    print("# long-stream parity: %d calls round robin over 4 blocks, %d Hz, %d-sample frames, one-channel contexts; RMS per block, device vs oracle"
          % (ls.CALLS, ls.SR, ls.FRAMES))
    if not args.no_repro:
        print("\n## 1. reproduction: full chain, %d taps (the gate's shape); the driver's flags compare calls 171-173, the default flags 226-228" % gl.REPRO_TAPS)
        for g in channels:
            rms, mx = gl.block_table(gl.device_prefix(g, ls.N_UNITS, gl.REPRO_TAPS), gl.oracle_repro(g))
            row("channel %d" % g, rms, mx)
            print("    blocks 168-175 rms: " + " ".join("%.2e" % v for v in rms[168:176]))
            print("    every block rms:    " + " ".join("%.1e" % v for v in rms))

    bounds = [ls.bound(k) for k in range(1, ls.N_UNITS + 1)]
    print("\n## 2. prefixes 1..8 of bench.CHAIN, %d taps; bound = 10 x the oracle's own worst-block spread on that prefix (floor 1e-15)" % args.taps)
    want = {}
    for g in channels:
        want[g] = ls.plain_stream(g) if args.taps == ls.TAPS else ls.prefix_stream(orc, g, taps=args.taps)
        for k in range(1, ls.N_UNITS + 1):
            got = gl.device_stream(pkg, g, bench.CHAIN[:k], args.taps, ls.input_blocks(g))
            rms, mx = gl.block_table(got, want[g][k])
            row("channel %3d prefix %d (.. %s)" % (g, k, bench.CHAIN[k - 1][0]), rms, mx, bounds[k - 1])

    print("\n## 3. every unit alone, fed the oracle's signal in front of it, %d taps" % args.taps)
    for g in channels:
        for k in range(1, ls.N_UNITS + 1):
            got = gl.device_stream(pkg, g, bench.CHAIN[k - 1:k], args.taps, want[g][k - 1])
            rms, mx = gl.block_table(got, want[g][k])
            row("channel %3d unit %d (%s)" % (g, k, bench.CHAIN[k - 1][0]), rms, mx, bounds[k - 1])

    print("\n## 4. the driver's control calls (set_overlap, profile_sample, profile_enable, profile_read) around its 174 calls, 6 channels, against plain calls")
    try:
        gl.test_the_drivers_control_calls_change_no_bit(pkg)
        print("bit-identical on all 174 calls: the control calls change nothing")
    except AssertionError as e:
        print("DIFFERS: (call, max_abs) = %s" % (e,))

    print("\n## 5. windows of 16 against per-frame calls, channel 0, full chain, %d taps" % ls.TAPS)
    try:
        gl.test_windows_of_16_give_the_bits_of_the_per_frame_stream(pkg)
        print("bit-identical on all %d blocks: batch mode shares whatever the per-frame stream shows" % ls.CALLS)
    except AssertionError as e:
        print("DIFFERS: (blocks, max_abs) = %s" % (e,))


if __name__ == "__main__":
    main()
