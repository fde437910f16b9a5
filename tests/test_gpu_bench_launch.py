"""`bench.py --gpus N` started WITHOUT a launcher must run N ranks (round-3 review: it ran one and printed "n_gpus": 1).  On the one-GPU box
both ranks share device 0 (GDG_BENCH_ONE_DEVICE=1): what is tested is the launch path, the rank bookkeeping and the line, not scaling."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_python_bench_gpus_2_prints_a_two_rank_line():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["GDG_BENCH_ONE_DEVICE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--channels", "64",
                        "--full", "--no-extras", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]                      # rank 0 alone prints
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["n_gpus_requested"] == 2
    assert [d["rank"] for d in line["devices"]] == [0, 1] and all(d["pci_bus_id"] for d in line["devices"])
    # the default job is FIXED (the reference's `-channels T`, controller.go:3262-3269): --channels 64 over two ranks = 32 each, strong scaling
    assert line["scaling"] == "strong" and line["config"]["total_channels"] == 64 and line["config"]["channels_per_gpu"] == 32
    assert line["settled"]["steps"] == 40 and line["settled"]["value"] > 0          # --steps 4: the settled figure rides on the same line
    assert line["parity"]["ok"] and line["parity"]["rms_max_all_ranks"] <= 1e-9
    assert line["value"] > 0 and line["roofline"]["frac"] is not None


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_are_refused_unless_asked_for():
    """Without GDG_BENCH_ONE_DEVICE the same command on a one-GPU box must NOT print a line that says "n_gpus": 2: the ranks exchange the PCI bus ids
    of their devices and stop when they are not distinct (on a box with two or more GPUs the ranks get a device each and the run succeeds)."""
    import torch
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "GDG_BENCH_ONE_DEVICE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--channels", "8", "--taps", "8192",
                        "--no-extras", "--no-cpu-baseline", "--no-parity"], env=env, capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if torch.cuda.device_count() >= 2:
        assert r.returncode == 0 and len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2
        assert len({d["pci_bus_id"] for d in json.loads(lines[0])["devices"]}) == 2
    else:
        assert r.returncode != 0 and not lines, r.stdout[-500:]
        assert "share 1 device" in r.stderr


def _oracle_output(oracle, bench, channel, blocks, frames, sr, taps, calls):
    """What the oracle's chain for `channel` returns on call number `calls`, fed the bench's round-robin input blocks."""
    ch = oracle.Chain()
    for name, p in bench.CHAIN:
        if isinstance(p, str):
            ch.append_unit(name, fir=bench.ir_for(p, channel, taps))
        else:
            ch.append_unit(name, params=p)
    for k in range(calls):
        want = ch.process(blocks[k % len(blocks)][channel], sr)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [1, 2])
def test_plain_run_prints_the_headline_alone_and_dumps_the_last_timed_step(tmp_path, oracle, gpus):
    """A plain run (no --full): exactly --steps timed steps and the headline, none of what --full measures besides.  --dump-outputs writes
    the output of the last timed step for every channel of the job, in global order (with two ranks on one device: gathered from both);
    the oracle, fed the same blocks for the same number of calls, gives the same samples."""
    import numpy as np
    import bench
    nch, frames, sr, taps, steps, warmup = 6, 1024, 48000, 4096, 3, 2
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    if gpus > 1:
        env["GDG_BENCH_ONE_DEVICE"] = "1"           # both ranks on device 0: what is tested is the gather of the rows, not scaling
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", str(steps), "--warmup", str(warmup),
                        "--channels", str(nch), "--frames", str(frames), "--sample-rate", str(sr), "--taps", str(taps),
                        "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["full"] is False and line["n_gpus"] == gpus and line["steps"] == steps and line["warmup"] == warmup
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f64" and line["value"] > 0
    assert abs(line["value"] - nch * frames / (line["ms_per_step"] * 1e-3) / 1e6) <= 1e-6 * line["value"]
    assert line["config"]["output_finite"] and line["config"]["total_channels"] == nch
    for key in ("ms_per_step_repeats", "roofline", "parity", "settled", "cpu_baseline", "end_to_end", "configs", "strong_split_legs", "one_gpu_alone"):
        assert key not in line, key
    assert line["outputs"]["channels"] == "all" and line["outputs"]["calls"] == warmup + steps
    assert sorted(os.listdir(out_dir)) == ["output.npy"]
    y = np.load(out_dir / "output.npy")
    assert y.dtype == np.float64 and y.shape == (nch, frames)
    blocks = bench.synth_blocks(nch, frames, sr)
    for c in (0, nch - 1):                      # with two ranks: one channel of each
        want = _oracle_output(oracle, bench, c, blocks, frames, sr, taps, warmup + steps)
        assert float(np.sqrt(np.mean((y[c] - want) ** 2))) <= 1e-9, c
