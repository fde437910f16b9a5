"""The three LFO-modulated delays (chorus, flanger, phaser) a third time, in plain Python floats, and a finder of the samples whose delay is a
WHOLE number of samples.

Written from the reference's Go (lines cited at each expression) and SURVEY.md Appendix B, operation for operation: IEEE-754 binary64, one
rounding per operation, no fused multiply-add.  The constants are Go's folded ones, read from oracle/go_consts.h (Go evaluates a constant
expression exactly and rounds once: 2 pi / 100 is not recomputed here).  No numpy in the arithmetic; numpy only makes the input blocks.

Why whole delays: the reference reads a fractional delay as  (1 - (d - floor d)) x[i - floor d] + (1 - (ceil d - d)) x[i - ceil d]
(flanger.go:66-97).  At a whole d, floor d == ceil d and both weights are 1: the delayed sample is counted TWICE.  A delay that is 1e-15 off
a whole number interpolates with weights (1, 1e-15) instead: the sample is counted once, and the output is wrong by wet mix x x[i - d].
Phases are rational fractions of a turn, so whole delays happen by construction (sin = -1, 0, 0.5, 1 on a sample), and a kernel that takes
its LFO by rotation instead of from sin() can miss them.

  stream(unit, params, sr, frames, inputs, calls)    the output blocks
  hits(unit, params, sr, frames, calls)              a Hit for every tap whose delay is whole, with two flags:
        robust      the delay is still whole with the sine moved by each of -2, -1, +1, +2 ulp (what another libm may return); sines of
                    exactly 0 and +-1 count as robust, the rule of oracle/libm_jitter.c
        sensitive   the delay is no longer whole with the sine moved by some value of +-2.2e-16 .. +-1e-15 absolute (what a rotated LFO is
                    off by): the hits a kernel can miss
    a hit that is not robust is FRAGILE: the Go binary's own answer depends on its libm there, and `stream(..., offsets=)` gives the answer
    for each ulp offset of that hit's sine.
"""
import collections
import math
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _go_consts():
    """{name: value} of oracle/go_consts.h (hexadecimal float literals: the exact binary64 values Go folds, effects/effects.go:48-56)"""
    out = {}
    with open(os.path.join(ROOT, "oracle", "go_consts.h")) as f:
        for m in re.finditer(r"^#define (GO_\w+) (\S+)", f.read(), re.M):
            out[m.group(1)] = float.fromhex(m.group(2))
    return out


_K = _go_consts()
TWO_PI = _K["GO_MATH_TWO_PI"]
TWO_PI_FIFTH = _K["GO_MATH_TWO_PI_FIFTH"]
TWO_PI_HUNDREDTH = _K["GO_MATH_TWO_PI_HUNDREDTH"]
PI_THOUSANDTH = _K["GO_MATH_PI_THOUSANDTH"]
DEGREE_TO_RADIANS = _K["GO_MATH_DEGREE_TO_RADIANS"]

Hit = collections.namedtuple("Hit", "call sample lfo delay sin robust sensitive")

ULP_OFFSETS = (-2, -1, 0, 1, 2)
ROTATION_ERRORS = tuple(s * v for v in (2.2e-16, 3.3e-16, 4.4e-16, 6.7e-16, 1e-15) for s in (-1.0, 1.0))


class _Setup:
    """what Process() derives from the parameters in front of its loop"""

    def __init__(self, unit, params, sr):
        self.unit = unit
        self.sr = float(sr)                                             # chorus.go:37, flanger.go:37, phaser.go:43
        if unit == "chorus":
            depth = 0.1 * float(params[0])                              # chorus.go:24
            self.depth = 0.0 if depth < 0.0 else (10.0 if depth > 10.0 else depth)      # chorus.go:29-33
            self.angular = PI_THOUSANDTH * float(params[1])             # chorus.go:35-36
            self.size = int(math.floor((0.05 * self.sr) + 0.5))         # chorus.go:38-39
            self.dry, self.wet = 0.5, 0.5                               # chorus.go:111
            self.lfos = 5
        elif unit in ("flanger", "phaser"):
            depth = 0.01 * float(params[0])                             # flanger.go:24, phaser.go:25-26
            self.depth = 0.0 if depth < 0.0 else (1.0 if depth > 1.0 else depth)        # flanger.go:29-33, phaser.go:31-35
            self.angular = TWO_PI_HUNDREDTH * float(params[1])          # flanger.go:35-36, phaser.go:37-38
            self.sr_inv = 1.0 / self.sr                                 # flanger.go:38, phaser.go:44
            self.size = int(math.floor((0.002 * self.sr) + 0.5))        # flanger.go:39-40, phaser.go:45-46
            self.dry, self.wet = 0.5, 0.5                               # flanger.go:98
            if unit == "phaser":
                radians = DEGREE_TO_RADIANS * float(params[2])          # phaser.go:39-40
                self.wet = 0.5 * math.sin(radians)                      # phaser.go:41  phaseFac
                self.dry = 1.0 - abs(self.wet)                          # phaser.go:42  phaseFacInv
            self.lfos = 1
        else:
            raise ValueError(unit)

    def sine(self, prev, i, j):
        """the LFO's sine of tap j at sample i of a call that starts at phase `prev`"""
        if self.unit == "chorus":
            time = float(i) / self.sr                                   # chorus.go:57-58   i / sr
            zero_phase = math.fmod(prev + (self.angular * time), TWO_PI)                # chorus.go:59-61
            phase = math.fmod(zero_phase + (TWO_PI_FIFTH * float(j)), TWO_PI)           # chorus.go:68-71
            return math.sin(phase)                                      # chorus.go:72
        time = float(i) * self.sr_inv                                   # flanger.go:58-59, phaser.go:64-65   i * (1 / sr)
        phase = math.fmod(prev + (self.angular * time), TWO_PI)         # flanger.go:60-62, phaser.go:66-68
        return math.sin(phase)                                          # flanger.go:63, phaser.go:69

    def delay(self, s):
        """the delay in samples for an LFO sine of s"""
        offset = self.depth * s                                         # chorus.go:72, flanger.go:63, phaser.go:69
        if self.unit == "chorus":
            return (0.001 * (40.0 + offset)) * self.sr                  # chorus.go:73-74
        return (0.001 * (self.depth + offset)) * self.sr                # flanger.go:64-65, phaser.go:70-71

    def next_phase(self, prev):
        """previousPhase after a call: it advances by the BUFFER's duration, whatever the frame length"""
        if self.unit == "chorus":
            buffer_time = float(self.size) / self.sr                    # chorus.go:114-115
            return math.fmod(prev + (self.angular * buffer_time), TWO_PI)               # chorus.go:116-118
        duration = float(self.size) * self.sr_inv                       # flanger.go:101-102, phaser.go:107-108
        return math.fmod(prev + (self.angular * duration), TWO_PI)      # flanger.go:103-105, phaser.go:109-111


def _shift(buf, x):
    """the delay buffer after a call (chorus.go:119-131, flanger.go:106-117, phaser.go:112-123)"""
    size, n = len(buf), len(x)
    boundary = size - n
    if boundary >= 0:
        buf[0:boundary] = buf[n:size]
        buf[boundary:size] = x
    else:
        buf[:] = x[-boundary:n]


def _tap(x, buf, i, d, missed):
    """one fractional read (chorus.go:75-108, flanger.go:66-97, phaser.go:72-103).  missed: what an interpolating reader gives whose delay is
    a rounding error away from this whole d: weights (1 - eps, eps), in the limit the sample once"""
    early, late = math.floor(d), math.ceil(d)
    idx_early, idx_late = i - int(early), i - int(late)
    s_early = x[idx_early] if idx_early >= 0 else buf[len(buf) + idx_early]
    s_late = x[idx_late] if idx_late >= 0 else buf[len(buf) + idx_late]
    if idx_early < 0:
        assert len(buf) + idx_early >= 0, (i, d)
    if idx_late < 0:
        assert len(buf) + idx_late >= 0, (i, d)
    if missed:
        assert early == late
        return s_early
    w_early = 1.0 - (d - float(early))
    w_late = 1.0 - (float(late) - d)
    return (w_early * s_early) + (w_late * s_late)


def move(v, k):
    """v moved by k ulp"""
    for _ in range(abs(k)):
        v = math.nextafter(v, math.inf if k > 0 else -math.inf)
    return v


def stream(unit, params, sr, frames, inputs, calls, offsets=None, missed=(), first=0, samples=None):
    """The unit's output blocks of calls first .. calls - 1 from zero state; call b is fed inputs[b % len(inputs)] (`frames` samples each).
    Calls in front of `first` only leave their state (the phase and the delay buffer: neither depends on an output).
    offsets: {(call, sample, lfo): k} moves that tap's sine by k ulp; missed: a set of (call, sample, lfo) read as an interpolating reader
    would (see _tap); samples: only these samples of each block are made (the others stay 0: no sample depends on another one's output)."""
    u = _Setup(unit, params, sr)
    offsets = offsets or {}
    missed = set(missed)
    blocks = [[float(v) for v in blk] for blk in inputs]
    assert all(len(blk) == frames for blk in blocks)
    buf = [0.0] * u.size                                                # chorus.go:47-51 (make: zeros)
    prev = 0.0
    out = []
    special = {(c, i) for (c, i, _) in list(offsets) + list(missed)}
    for call in range(calls):
        x = blocks[call % len(blocks)]
        if call >= first:
            y = [0.0] * frames
            for i in (range(frames) if samples is None else samples):
                plain = (call, i) not in special
                if u.lfos == 1:
                    s = u.sine(prev, i, 0)
                    if not plain:
                        s = move(s, offsets.get((call, i, 0), 0))
                    delayed = _tap(x, buf, i, u.delay(s), (not plain) and (call, i, 0) in missed)
                else:
                    delayed = 0.0
                    for j in range(5):                                  # chorus.go:67
                        s = u.sine(prev, i, j)
                        if not plain:
                            s = move(s, offsets.get((call, i, j), 0))
                        delayed += 0.2 * _tap(x, buf, i, u.delay(s), (not plain) and (call, i, j) in missed)    # chorus.go:108
                y[i] = (u.dry * x[i]) + (u.wet * delayed)               # chorus.go:111, flanger.go:98, phaser.go:104
            out.append(y)
        prev = u.next_phase(prev)
        _shift(buf, x)
    return out


def classify(u, s):
    """(robust, sensitive) of a tap whose sine s gives a whole delay"""
    def whole(v):
        d = u.delay(v)
        return d == math.floor(d)
    robust = s in (0.0, 1.0, -1.0) or all(whole(move(s, k)) for k in ULP_OFFSETS if k)
    sensitive = any(not whole(s + e) for e in ROTATION_ERRORS)
    return robust, sensitive


def hits(unit, params, sr, frames, calls):
    """[Hit] in stream order: every tap of the stream whose delay is a whole number of samples"""
    u = _Setup(unit, params, sr)
    found = []
    prev = 0.0
    for call in range(calls):
        for i in range(frames):
            for j in range(u.lfos):
                s = u.sine(prev, i, j)
                d = u.delay(s)
                if d == math.floor(d):
                    found.append(Hit(call, i, j, int(d), s, *classify(u, s)))
        prev = u.next_phase(prev)
    return found


def block_inputs(seed, frames, blocks=4):
    """[blocks][frames] numpy: every sample +-(0.25 .. 0.9), sign and magnitude from the reference's LCG (helpers.lcg_floats) -- no sample
    near zero, so a delayed sample counted once instead of twice moves the output by at least 0.25 x the wet mix"""
    import numpy as np
    from helpers import lcg_floats
    n = frames * blocks
    mag = 0.25 + 0.65 * lcg_floats(seed, n)
    sign = np.where(lcg_floats(seed + 7919, n) < 0.5, -1.0, 1.0)
    return (sign * mag).reshape(blocks, frames)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
# (unit, params, sr, frames, calls), and per case the hits the finder has to return among its own: (call, sample, lfo, delay, fragile).
# Every row keeps speed within the reference's range 1 .. 100.  The call counts run a few calls past the first robust hit of a row, so that
# every case holds at least two robust, sensitive hits besides (0, 0) and no more fragile hits than robust ones: the depth-100 flanger rows
# cross sin = 0.5 (72 or 288 samples, fragile, some 35 calls in a row) on the way to sin = 1 (the ring capacity, robust), so they run on
# into the sin = 1 calls until those outnumber the fragile ones.
Case = collections.namedtuple("Case", "unit params sr frames calls expect")

_FLANGER_ROWS = [
    # 8192 frames: thread 992 reaches sample 8160 after 7 rotations of its LFO
    ((100, 100), 48000, 8192, 80, [(0, 4000, 0, 72, True), (40, 8160, 0, 96, False), (41, 8064, 0, 96, False), (79, 4416, 0, 96, False)]),
    # a delay of 0, reached from below: sin = -1
    ((40, 100), 48000, 8192, 293, [(290, 8160, 0, 0, False), (291, 8064, 0, 0, False), (292, 7968, 0, 0, False)]),
    # every sample below index 1024: no rotation, the device's sincos alone
    ((100, 100), 48000, 512, 371, [(40, 160, 0, 72, True), (120, 480, 0, 96, False), (125, 0, 0, 96, False), (370, 480, 0, 0, False)]),
    # odd samples.  Depth 99, not 100: at 44.1 kHz depth 100 reaches a delay of 88.2 samples in a buffer of 88, and where that happens at
    # sample 0 of a call (calls 118 .. 132 of this stream) the reference indexes its buffer at -1 and panics; the oracle reads past its
    # buffer there and the kernel wraps round its ring.  No implementation has an answer to compare.  Depth 99 stays inside the buffer
    # (87.3 samples) and keeps the row's hits: 0.99 + 0.99 sin is 0 at sin = -1 on the same samples
    ((99, 100), 44100, 8192, 286, [(283, 8171, 0, 0, False), (284, 8083, 0, 0, False), (285, 7995, 0, 0, False)]),
    ((100, 100), 192000, 8192, 120, [(21, 7936, 0, 288, True), (104, 8064, 0, 384, False), (119, 2304, 0, 384, False)]),
]

CASES = [Case("flanger", list(p), sr, frames, calls, expect) for p, sr, frames, calls, expect in _FLANGER_ROWS]
# the phaser on the same streams: phaseFac 0.5 at 90 degrees, -0.433 at -60
CASES += [Case("phaser", list(p) + [phase], sr, frames, calls, expect)
          for phase, rows in ((90, (0, 2, 4)), (-60, (1, 2, 3))) for p, sr, frames, calls, expect in (_FLANGER_ROWS[r] for r in rows)]
CASES += [
    Case("chorus", [100, 100], 48000, 8192, 31, [(0, 0, 0, 1920, False), (4, 6400, 2, 2160, False), (17, 7200, 1, 2400, False), (30, 8000, 0, 2160, True)]),
    Case("chorus", [100, 100], 192000, 8192, 34, [(6, 6400, 2, 8640, False), (20, 0, 1, 9600, False), (33, 3200, 0, 8640, True)]),
    Case("chorus", [100, 100], 44100, 8192, 20, [(17, 6615, 1, 2205, False), (18, 4410, 1, 2205, False), (19, 2205, 1, 2205, False)]),
    # a frame that is no multiple of 1024 (nor of the 512 threads of the two-per-CU build): the kernels' loop with a remainder
    Case("chorus", [100, 100], 48000, 5000, 40, [(5, 4000, 2, 2160, False), (18, 4800, 1, 2400, False), (32, 3200, 0, 2160, True), (38, 4800, 2, 1920, False)]),
]

# the neighbour channel of the GPU test: the same unit with no whole delay in its stream (the chorus: none but sample 0 of call 0, sin(0))
QUIET = {"flanger": [35, 77], "phaser": [35, 77, 30], "chorus": [35, 77]}


def case_id(case):
    return "%s-%s-%d-%d" % (case.unit, "_".join(str(p) for p in case.params), case.sr, case.frames)


def case_seed(case):
    return 9001 + 13 * CASES.index(case)
