"""The frame-length schedule of test_frame_lengths_host.py and test_gpu_frame_lengths.py (calls nothing of the library).

One stream per sample rate, cut into calls whose lengths are the ones the general segment kernel has code for and the fixed-size tests never
reach: scans of one element and part-filled first waves (1, 2, 3, 63, 65), ragged chunks with a partly filled last thread and empty threads
behind it (1025, 2049, 3000, 4097, 8191: m = (N + 1023) / 1024 >= 2), and every delay ring's capacity C with both neighbours -- the
reference's buffer shift has a branch for N <= C and one for N > C (effects/autoyoy.go:145-155)."""

RATES = (22050, 48000, 192000)          # not 44100: flanger depth 100 indexes the reference's 88-sample buffer at -1 there
MAX_FRAMES = 8192
HEAD = [1, 2, 3, 1, 63, 64, 65, 1023, 1025, 2047, 2049, 3000, 4097, 8191, 8192, 7]
TAIL = [8191, 1, 2]
# ring capacities in seconds: flanger and phaser, delay at 3 ms (("delay", [3, -10, 0])), auto-yoy, chorus
RING_SECONDS = (0.002, 0.003, 0.01, 0.05)


# Where the reference has no output.  An oversampled shaper or fuzz decimates through filter.Process with its anti-aliasing taps
# (oversampling/oversampling.go:149-150) on the F N oversampled samples of the call, and filter.Process panics on a slice bound when
# F N is not a power of two and a block of nextpow2(taps) samples starts beyond it (filter/filter.go:370-382, :443-453) -- the pairs the
# library rejects for power amps.  OVERSAMPLING_PARAM: the index of the unit's "oversampling" parameter (0: none, 1: 2x, 2: 4x);
# AA_TAPS: the decimator's filter length per factor (oversampling.go:239-317, :357-513).
OVERSAMPLING_PARAM = {"overdrive": 5, "distortion": 3, "excess": 2, "fuzz": 6}
AA_TAPS = {2: 77, 4: 155}


def oversampling_factor(unit, params):
    if unit not in OVERSAMPLING_PARAM or params is None:
        return 1                            # the default of all four is no oversampling
    return 1 << params[OVERSAMPLING_PARAM[unit]]


def decimator_pair(unit, params, n):
    """(frames, taps) the reference's filter.Process sees inside the unit at a call of n samples, or None without oversampling"""
    f = oversampling_factor(unit, params)
    return (f * n, AA_TAPS[f]) if f > 1 else None


def ring_capacities(sr):
    """math.Floor(seconds * sampleRate + 0.5) of the reference, sorted"""
    return sorted({int(s * sr + 0.5) for s in RING_SECONDS})


def schedule(sr):
    out = list(HEAD)
    for c in ring_capacities(sr):
        if c + 1 <= MAX_FRAMES:
            out += [c - 1, c, c + 1]
    return out + list(TAIL)
