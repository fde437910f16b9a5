"""The numpy restatement of the dither arithmetic include/gdg.h states (gdg_batch_set_dither): what tests/test_dither_host.py holds the
header's host form against and tests/test_gpu_dither.py the kernels, byte for byte.  Nothing here calls the code under test."""
import numpy as np

K, M0, M1 = 0x9e3779b97f4a7c15, 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
MASK = (1 << 64) - 1
PORT_LEFT, PORT_RIGHT, PORT_METRONOME = 0xfffffffd, 0xfffffffe, 0xffffffff
SCALE = {"lpcm8": 127.0, "lpcm16": 32767.5, "lpcm24": 8388607.5, "lpcm32": 2147483647.5}
RANGE = {"lpcm8": (-128, 127), "lpcm16": (-32768, 32767), "lpcm24": (-8388608, 8388607), "lpcm32": (-2147483648, 2147483647)}
WIDTH = {"lpcm8": 1, "lpcm16": 2, "lpcm24": 3, "lpcm32": 4}

# the issue's known answers: seed, port, index, x -> h, LPCM16 code, LPCM24 code
KNOWN = [
    (0x0, 0, 0, 0.0, 0xdf9545e13007448a, 1, 1),
    (0x1, 0, 0, 0.25, 0x8dde58528d955053, 8192, 2097152),
    (0x3039, 7, 0xffffffff, 0.25, 0xebb51d375a797963, 8192, 2097152),
    (0x3039, 7, 0x100000000, -0.7, 0xe8f8277b0aa97796, -22936, -5872024),
    (0xdeadbeefcafef00d, 0xfffffffd, 2 ** 40 + 1, 1.5, 0x71a1a79a27a98aec, 32767, 8388607),
    (0x63, 3, 8191, -1.0, 0xaedc319de87b0798, -32768, -8388608),
    (0x63, 3, 8192, 1e-5, 0x33a34e84d34b5c4b, 0, 83),
]


def fmix_int(x):
    x ^= x >> 33
    x = (x * M0) & MASK
    x ^= x >> 33
    x = (x * M1) & MASK
    return x ^ (x >> 33)


def key_of(seed, port):
    return fmix_int((seed + (port + 1) * K) & MASK)


def fmix(x):
    """x: uint64 array; numpy's uint64 arithmetic is modulo 2^64"""
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(M0)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(M1)
    return x ^ (x >> np.uint64(33))


def hashes(seed, port, first, n):
    with np.errstate(over="ignore"):
        index = np.uint64(first & MASK) + np.arange(n, dtype=np.uint64)
        return fmix((index + np.uint64(K)) ^ np.uint64(key_of(seed, port)))


def noise(seed, port, first, n):
    """d of the samples [first, first + n) of a port: triangular on (-1, 1)"""
    h = hashes(seed, port, first, n)
    a, b = (h >> np.uint64(32)).astype(np.int64), (h & np.uint64(0xffffffff)).astype(np.int64)
    return (a - b).astype(np.float64) * 2.0 ** -32


def codes(fmt, x, seed, port, first=0):
    """the signed codes (int64) of a row of float64 samples"""
    x = np.asarray(x, dtype=np.float64)
    t = SCALE[fmt] * np.clip(x, -1.0, 1.0)
    q = np.floor((t + noise(seed, port, first, x.size)) + 0.5)          # two adds, each rounded on its own: numpy never fuses
    lo, hi = RANGE[fmt]
    return np.clip(q, lo, hi).astype(np.int64)


def encode(fmt, x, seed, port, first=0):
    """the file's bytes (uint8 array) of a row"""
    q = codes(fmt, x, seed, port, first)
    if fmt == "lpcm8":
        return np.clip(q + 128, 0, 255).astype(np.uint8)
    w = WIDTH[fmt]
    return np.ascontiguousarray((q & 0xffffffff).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :w]).reshape(-1)


def decode_codes(fmt, data):
    """the signed codes back from a file's bytes"""
    data = np.asarray(data, dtype=np.uint8)
    if fmt == "lpcm8":
        return data.astype(np.int64) - 128
    w = WIDTH[fmt]
    b = np.zeros((data.size // w, 4), dtype=np.uint8)
    b[:, :w] = data.reshape(-1, w)
    v = b.reshape(-1).view("<u4").astype(np.int64)
    bits = 8 * w
    return np.where(v >= 1 << (bits - 1), v - (1 << bits), v)
