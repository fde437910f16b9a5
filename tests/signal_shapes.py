"""The signal family of test_signal_shapes_host.py and test_gpu_signal_shapes.py (numpy and helpers.synth_signal; calls nothing of the library).

Every other parity test feeds the kernels helpers.synth_signal -- two sines and 5 % noise, peak about 0.8 -- scaled by at most 1.0.  These are
the inputs that family never is: above full scale, at and below the smallest normal double, exactly zero, exactly +-1.0, DC, one non-zero
sample.  Positions are given in calls of `frames` samples, so they follow the block size in use."""
import functools
from collections import OrderedDict

import numpy as np

from helpers import synth_signal

# (rate, frames per call, calls): the full-frame register paths at two rates and the general ragged path
PAIRS = ((48000, 8192, 4), (22050, 1000, 6), (192000, 8192, 4))
SQUARE_PERIOD = 74
NAMES = ("loud8", "loud1000", "tiny", "subnormal", "silence", "burst_then_silence", "silence_then_burst", "impulse", "dc", "step",
         "square_full_scale", "nyquist", "negative_zero_run")


def impulse_at(frames):
    """the one non-zero sample of `impulse`: inside call 1, off every power of two"""
    return frames + frames // 3


@functools.lru_cache(maxsize=None)
def base_signal(channel, n, sr):
    """synth_signal(channel, n, sr), made once and read-only"""
    x = synth_signal(channel, n, sr)
    x.setflags(write=False)
    return x


def signals(channel, n, sr, frames):
    """name -> float64 [n], in the order of NAMES; base = synth_signal(channel, n, sr)"""
    base = base_signal(channel, n, sr)
    out = OrderedDict()
    out["loud8"] = 8.0 * base
    out["loud1000"] = 1000.0 * base
    out["tiny"] = 1e-12 * base
    out["subnormal"] = 1e-305 * base
    out["silence"] = np.zeros(n)
    x = base.copy()
    x[frames + frames // 2:] = 0.0
    out["burst_then_silence"] = x
    x = base.copy()
    x[:2 * frames + frames // 2] = 0.0
    out["silence_then_burst"] = x
    x = np.zeros(n)
    x[impulse_at(frames)] = 1.0
    out["impulse"] = x
    out["dc"] = np.full(n, 0.5)
    x = np.full(n, -0.25)
    x[frames + (2 * frames) // 5:] = 0.75
    out["step"] = x
    out["square_full_scale"] = np.where((np.arange(n) % SQUARE_PERIOD) < SQUARE_PERIOD // 2, 1.0, -1.0)
    out["nyquist"] = np.where(np.arange(n) % 2 == 0, 0.9, -0.9)
    x = base.copy()
    x[frames + frames // 4:3 * frames + frames // 4] = -0.0
    out["negative_zero_run"] = x
    assert tuple(out) == NAMES
    for v in out.values():
        assert v.dtype == np.float64 and v.shape == (n,)
    return out


def row_channel(k):
    """the synth_signal channel of UNIT_CASES row k (as in test_gpu_frame_lengths.oracle_stream)"""
    return 7 * k + 3


def oracle_row(oracle, unit, params, x, cuts, sr):
    """One unit on the oracle handed in, x cut into `cuts`"""
    ch = oracle.Chain()
    ch.append_unit(unit, params=params)
    out, pos = [], 0
    for n in cuts:
        out.append(ch.process(x[pos:pos + n], sr))
        pos += n
    assert pos == x.size
    return np.concatenate(out)


def key(unit, params):
    return (unit, None if params is None else tuple(params))


# (unit, params, signal, rate) at which the oracle's own output moves by more than 1e-10 * max(1, peak |want|) under x * (1 + 2**-50): no
# yardstick at 1e-9.  Pinned to the measurement by test_signal_shapes_host.py; held to shape and finiteness only by
# test_gpu_signal_shapes.py.  Measured on all 60 rows x 13 signals x 3 pairs: none.  The fold of `excess` (effects/excess.go:33-63) is
# ill-conditioned in proportion to the amplitude, but at 1000 x base and the 20, 30 and 12 dB of the three rows it stays below the bar, so
# loud1000 keeps its gain of 1000 at every rate.
ILL_CONDITIONED = {}

# Rows of test_frame_lengths_host.CUT_INVARIANT whose oracle output does depend on the cut at one of PAIRS: (unit, params, rate) ->
# (the samples that differ between calls of `frames` and calls of 1024, reason).  The same for every signal: the generator does not
# look at its input.  test_gpu_signal_shapes.py cuts its reference as it cuts the kernel's stream, so it holds these rows as all others.
CUT_EXCEPTIONS = {
    ("signal_generator", (100, 0, 2, 123, 50, 0), 22050): (
        [3675], "123 Hz at 22050 Hz: sample 3675 is 20.5 periods, sign(pi - phase) sits on its jump and the phase is rounded once per call, "
                "fmod(phase + N * increment) (effects/signalgenerator.go:96-98, :102-103)"),
}

# Part (c), one non-finite sample: rows of CUT_INVARIANT (none is oversampled) for which the reference has no output to compare with.
POISON_AT = 300                 # the poisoned sample of call 1 (0-based)
POISON_DROPPED = {
    ("auto_yoy", None): "the level of a NaN envelope is NaN, neither <= A nor >= B, so the delay is NaN and the buffer is indexed by "
                        "i - int(NaN): the reference panics (effects/autoyoy.go:90-124); +inf turns the level follower's envelope into NaN "
                        "one sample later (inf - inf, :83-85)",
    ("auto_yoy", (0, -10, -50, 40)): "as above with the peak follower: envelope *= d makes the state NaN and sampleAbs > NaN is false for ever "
                                     "(effects/autoyoy.go:72-81, :90-124); the row is dropped for +inf with it, one reason per row",
}
