"""bench.py --dump-outputs on CPU: which channels are written, in which order, and the size limit (the GPU side:
tests/test_gpu_bench_launch.py)."""
import numpy as np

import bench


class _TwoRanks:
    """gather_object of a two-rank gloo group, seen from rank 0: rank 1's part is given up front."""

    def __init__(self, other):
        self.other = other

    def get_world_size(self):
        return 2

    def gather_object(self, obj, object_gather_list, dst=0):
        object_gather_list[0], object_gather_list[1] = self.other, obj


def test_every_channel_in_global_order_below_the_limit(tmp_path):
    y = np.arange(6 * 8, dtype=np.float64).reshape(6, 8)
    info = bench.dump_outputs(str(tmp_path), y, 0, 6, 0)
    assert info["channels"] == "all" and info["files"] == {"output.npy": [6, 8]} and info["dtype"] == "float64"
    got = np.load(tmp_path / "output.npy")
    assert got.dtype == np.float64 and np.array_equal(got, y)


def test_rows_of_two_ranks_are_put_in_channel_order(tmp_path):
    y = np.random.default_rng(1).standard_normal((8, 16))
    # rank 0 holds channels 0..3, rank 1 channels 4..7; the gathered list need not arrive in rank order
    info = bench.dump_outputs(str(tmp_path), y[:4], 0, 8, 0, dist=_TwoRanks((4, y[4:])))
    assert info["channels"] == "all"
    assert np.array_equal(np.load(tmp_path / "output.npy"), y)
    assert bench.dump_outputs(str(tmp_path / "other"), y[4:], 4, 8, 1, dist=None) is None          # only rank 0 writes


def test_a_larger_job_is_a_fixed_seeded_sample_within_64_mb():
    frames = 8192
    assert len(bench.dump_channels(1024, frames)) == 1024                   # 1024 x 8192 float64 = 64 MB: everything
    a, b = bench.dump_channels(4096, frames), bench.dump_channels(4096, frames)
    assert np.array_equal(a, b) and len(a) * frames * 8 <= 64 << 20 and len(a) == 1024
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 4096
