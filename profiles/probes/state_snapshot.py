"""Channel state save / load (gdg_state_*) on the bench chain at 192 kHz, 8192-sample frames: bytes per channel,
device save / load time and bandwidth (read + write), host save / load time.  Run on the GPU box:
    python profiles/probes/state_snapshot.py [--channels 64,512] [--reps 10]
One line per channel count on stdout."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry                                   # noqa: E402
from helpers import synth_ir, synth_signal                        # noqa: E402

FRAMES, SR, TAPS = 8192, 192000, 65536
CHAIN = [("compressor", [1, 30, -20]), ("overdrive", [0, 20, 100, 0, 1, 0]), ("tone_stack", None), ("chorus", None),
         ("power_amp", 5), ("power_amp", 6), ("cabinet", None), ("reverb", [50])]


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", default="64,512")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    pkg = entry.load_package()
    irs = {s: synth_ir(TAPS, seed=s) for s in (5, 6)}
    for nch in [int(v) for v in a.channels.split(",")]:
        ctx = pkg.Context(nch, FRAMES)
        if nch >= 384:
            ctx.set_overlap(2)
        for c in range(nch):
            for name, p in CHAIN:
                if isinstance(p, int):
                    ctx.append_unit(c, name, fir=irs[p])
                else:
                    ctx.append_unit(c, name, params=p)
        d_in, d_out = ctx.alloc(nch, FRAMES), ctx.alloc(nch, FRAMES)
        d_in.upload(np.stack([synth_signal(c, FRAMES, SR) for c in range(nch)]))
        for _ in range(10):
            ctx.process_device(d_in, d_out, FRAMES, SR)
        ctx.synchronize()
        size = ctx.state_size()
        blob_dev = ctx.alloc(1, (size + 7) // 8)
        t_save_dev = timed(lambda: ctx.save_state_device(blob_dev), a.reps)
        t_load_dev = timed(lambda: ctx.load_state_device(blob_dev, size), a.reps)
        blob = ctx.save_state()
        t_save_host = timed(ctx.save_state, max(3, a.reps // 3))
        t_load_host = timed(lambda: ctx.load_state(blob), max(3, a.reps // 3))
        moved = 2.0 * size                                        # read + write
        print("channels=%d bytes=%d bytes_per_channel=%d save_device_us=%.1f (%.2f TB/s) load_device_us=%.1f (%.2f TB/s) "
              "save_host_us=%.1f load_host_us=%.1f" % (nch, size, size // nch, t_save_dev, moved / t_save_dev / 1e6, t_load_dev,
                                                      moved / t_load_dev / 1e6, t_save_host, t_load_host), flush=True)
        blob_dev.free()
        d_in.free()
        d_out.free()
        ctx.close()


if __name__ == "__main__":
    main()
