"""The launch shape each step ran in, read from GDG_PLAN_TRACE=2 (one [launch] line per step launch, process_rows), just below and just above
every threshold of decide_shapes (api_plan.cpp) at the options' defaults.  The bit-identity tests compare an option on against off and would
pass if the "on" run fell back to the plain shape; these tests pin which shape runs."""
import numpy as np
import pytest

import __graft_entry__ as entry
from helpers import launches, synth_ir, synth_signal

pytestmark = pytest.mark.gpu
FRAMES = 8192
TAPS = 65536                                      # 8 partitions per power amp at 8192-sample frames

HEAD = [("compressor", [1, 30, -20]), ("overdrive", [0, 20, 100, 0, 1, 0]), ("tone_stack", None), ("chorus", None)]
ONE_AMP = HEAD + [("power_amp", "a"), ("cabinet", None)]
BENCH = HEAD + [("power_amp", "a"), ("power_amp", "b"), ("cabinet", None), ("reverb", [50])]
RELEASE = [("flanger", None), ("delay", None), ("octaver", None), ("power_amp", "a"), ("phaser", None)]
CONFIG3 = [("compressor", [1, 30, -20]), ("overdrive", [0, 20, 100, 0, 1, 2]), ("tone_stack", None), ("power_amp", "a"), ("cabinet", None),
           ("reverb", [50])]


@pytest.fixture(scope="module")
def pkg():
    return entry.load_package()


@pytest.fixture(scope="module")
def irs():
    return {k: synth_ir(TAPS, seed=s) for k, s in (("a", 5), ("b", 6))}


def trace(pkg, irs, capfd, monkeypatch, nch, chain, sr=192000, calls=2, window=0, groups=0, options=None, flanger_in=None, taps=TAPS):
    """the [launch] lines of each of `calls` per-frame calls (or one window of `window` frames)"""
    monkeypatch.setenv("GDG_PLAN_TRACE", "2")
    ctx = pkg.Context(nch, FRAMES)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    if groups:
        ctx.set_overlap(groups)
    for c in range(nch):
        for name, p in chain:
            if name == "chorus" and c == flanger_in:
                name, p = "flanger", None
            if isinstance(p, str):
                ctx.append_unit(c, name, fir=irs[p][:taps])
            else:
                ctx.append_unit(c, name, params=p)
    x = np.stack([synth_signal(c, FRAMES * max(window, 1), sr) for c in range(nch)])
    d_in, d_out = ctx.alloc(nch, FRAMES * max(window, 1)), ctx.alloc(nch, FRAMES * max(window, 1))
    d_in.upload(x)
    capfd.readouterr()
    out = []
    if window:
        ctx.set_window(window)
        ctx.process_window_device(d_in.ptr, d_out.ptr, window * FRAMES, window, sr)
        ctx.synchronize()
        out.append(launches(capfd.readouterr().err))
    for _ in range(calls if not window else 0):
        ctx.process_device(d_in, d_out, FRAMES, sr)
        ctx.synchronize()
        out.append(launches(capfd.readouterr().err))
    ctx.close()
    return out


def step_shapes(lines, drop_premac=True):
    """[shape of step 0, step 1, ...] of one call (group 0)"""
    return [r["shape"] for r in lines if r["group"] == 0 and not (drop_premac and r["shape"] == "PREMAC")]


@pytest.mark.parametrize("nch,chain,fir", [(112, ONE_AMP, "SPLIT"), (128, ONE_AMP, "FUSED"), (192, BENCH, "SPLIT"), (208, BENCH, "FUSED")])
def test_split_or_fused_convolution_by_channels_and_amps(pkg, irs, capfd, monkeypatch, nch, chain, fir):
    first = trace(pkg, irs, capfd, monkeypatch, nch, chain, calls=1)[0]
    assert {r["shape"] for r in first if r["shape"] in ("SPLIT", "SPLIT_PREMAC", "FUSED")} == {fir}


def test_premac_is_used_from_the_second_call(pkg, irs, capfd, monkeypatch):
    one, two = trace(pkg, irs, capfd, monkeypatch, 64, BENCH)
    assert step_shapes(one) == ["SEGT", "SPLIT", "SPLIT", "SEGT"]
    assert [r["step"] for r in one if r["shape"] == "PREMAC"] == [1, 2]
    assert step_shapes(two) == ["SEGT", "SPLIT_PREMAC", "SPLIT_PREMAC", "SEGT"]
    assert [r["chained"] for r in two if r["step"] in (1, 2) and r["shape"] != "PREMAC"] == [0, 1]


def test_no_premac_below_the_partition_minimum(pkg, irs, capfd, monkeypatch):
    """32 channels x 8 partitions with one amp: 256 < 384"""
    one, two = trace(pkg, irs, capfd, monkeypatch, 32, ONE_AMP)
    for call in (one, two):
        assert "PREMAC" not in {r["shape"] for r in call}
        assert step_shapes(call)[1] == "SPLIT"


@pytest.mark.parametrize("nch,seg", [(112, "SEGT"), (128, "SEGF")])
def test_two_per_cu_kernel_from_128_channels(pkg, irs, capfd, monkeypatch, nch, seg):
    call = trace(pkg, irs, capfd, monkeypatch, nch, ONE_AMP, calls=1)[0]
    assert step_shapes(call)[0] == seg


def test_general_kernel_at_112_channels_without_tiles(pkg, irs, capfd, monkeypatch):
    call = trace(pkg, irs, capfd, monkeypatch, 112, ONE_AMP, calls=1, options={"seg_tile_max_channels": 0})[0]
    assert step_shapes(call)[0] == "GENERAL"


def test_tiles_and_reverb_ahead_for_the_bench_chain_at_64(pkg, irs, capfd, monkeypatch):
    call = trace(pkg, irs, capfd, monkeypatch, 64, BENCH, calls=1)[0]
    assert call[0]["shape"] == "SEGT" and call[0]["ahead"] == 64
    assert call[3]["shape"] == "SEGT"


def test_one_flanger_keeps_the_step_on_the_general_kernel(pkg, irs, capfd, monkeypatch):
    call = trace(pkg, irs, capfd, monkeypatch, 8, ONE_AMP, calls=1, flanger_in=3, taps=16384)[0]
    assert step_shapes(call)[0] == "GENERAL" and step_shapes(call)[2] == "SEGT"


@pytest.mark.parametrize("nch,seg,ahead", [(72, "SEGT", 72), (80, "GENERAL", 0)])
def test_two_premac_amps_take_tiles_and_reverb_ahead_off_above_72(pkg, irs, capfd, monkeypatch, nch, seg, ahead):
    call = trace(pkg, irs, capfd, monkeypatch, nch, BENCH, calls=1)[0]
    assert step_shapes(call) == [seg, "SPLIT", "SPLIT", seg]
    assert call[0]["ahead"] == ahead


@pytest.mark.parametrize("nch,ahead", [(112, 112), (127, 127), (128, 0)])
def test_reverb_ahead_up_to_127_channels_without_premac(pkg, irs, capfd, monkeypatch, nch, ahead):
    call = trace(pkg, irs, capfd, monkeypatch, nch, BENCH, calls=1, options={"fir_premac": 0})[0]
    assert call[0]["ahead"] == ahead
    if ahead:
        assert call[0]["shape"] == "GENERAL_AHEAD"            # 2 x channels + the reverbs' workgroups exceed the tile budget


def test_config3_compressor_runs_inside_the_oversampled_shaper_launch(pkg, irs, capfd, monkeypatch):
    call = trace(pkg, irs, capfd, monkeypatch, 64, CONFIG3, sr=96000, calls=1, taps=32768)[0]
    assert step_shapes(call)[:3] == ["SKIP", "OS_TILES_PREFIX", "SEGT"]
    window = trace(pkg, irs, capfd, monkeypatch, 64, CONFIG3, sr=96000, window=2, taps=32768)[0]
    assert step_shapes(window)[:2] == ["WAVE", "OS_TILES"]


@pytest.mark.parametrize("nch,seg", [(448, "SEGF_WAVE"), (512, "SEGF_WALK")])
def test_windows_run_a_workgroup_per_frame_up_to_448_channels(pkg, irs, capfd, monkeypatch, nch, seg):
    call = trace(pkg, irs, capfd, monkeypatch, nch, ONE_AMP, window=2, taps=8192)[0]
    assert step_shapes(call) == [seg, "FIR_WINDOW", seg]


@pytest.mark.parametrize("nch,seg", [(112, "WAVE"), (128, "WALK")])
def test_windows_with_a_release_unit_only_up_to_112_channels(pkg, irs, capfd, monkeypatch, nch, seg):
    call = trace(pkg, irs, capfd, monkeypatch, nch, RELEASE, window=2, taps=8192)[0]
    assert step_shapes(call) == [seg, "FIR_WINDOW", seg]


def test_two_groups_take_no_tiles_premac_or_absorbed_compressor(pkg, irs, capfd, monkeypatch):
    for chain, kw in ((BENCH, {}), (CONFIG3, {"sr": 96000, "taps": 32768})):
        for call in trace(pkg, irs, capfd, monkeypatch, 64, chain, groups=2, **kw):
            assert {r["group"] for r in call} == {0, 1}
            assert all(r["n"] == 32 and r["ahead"] == 0 for r in call)
            assert not {r["shape"] for r in call} & {"SEGT", "SPLIT_PREMAC", "PREMAC", "SKIP", "OS_TILES_PREFIX", "GENERAL_AHEAD"}
