"""gdg_batch_stream_span: which source frames a range of the job's output samples reads -- pure arithmetic, checked without a device
against a plain-Python restatement of resample.Time's indexing (resample/resample.go:36-103):

    out_len = floor(n * dst / src), one less when that product is whole (:72-87); dx = src / dst (:88-90);
    output i reads the source indices j = floor(i * dx) - 2 .. floor(i * dx) + 3 that lie in [0, n) (:91-103).

The products are float64 products in the reference, so they are here (Python floats)."""
import math

import numpy as np
import pytest

import __graft_entry__ as entry

BLOCK = 8192
RATES = [44100, 48000, 88200, 96000, 192000, 8000, 11025, 22050, 37800, 47999, 176400]


@pytest.fixture(scope="module")
def pkg():
    return entry.load_package()


def out_length(n, src, dst):
    f = float(n) * (float(dst) / float(src))
    fl = math.floor(f)
    return max(int(fl) - (1 if fl == f else 0), 0)


def reads(i, n, src, dst):
    """the source indices output sample i reads"""
    idx = math.floor(float(i) * (float(src) / float(dst)))
    return [j for j in range(idx - 2, idx + 4) if 0 <= j < n]


def want_span(n, src, dst, first, count):
    """hull of what outputs [first, first + count) read: only the two ends matter, floor(i * dx) is monotone in i"""
    covered = n if src == dst else out_length(n, src, dst)
    a, b = first, min(first + count, covered)
    if a >= b:
        return None
    if src == dst:
        return a, b
    return reads(a, n, src, dst)[0], reads(b - 1, n, src, dst)[-1] + 1


def random_slicing(rng, blocks):
    cuts, left = [], blocks
    while left:
        k = int(min(left, rng.integers(1, 7)))
        cuts.append(k)
        left -= k
    return cuts


@pytest.mark.parametrize("seed", range(24))
def test_span_covers_what_the_formula_reads_and_slices_hand_every_frame_over_once(pkg, seed):
    rng = np.random.default_rng(500 + seed)
    dst = int(rng.choice(RATES[:5]))
    src = int(rng.choice(RATES))
    n = int(rng.choice([1, 5, 6, 7, 100, BLOCK - 1, BLOCK, BLOCK + 1, int(rng.integers(2, 200000))]))
    covered = n if src == dst else out_length(n, src, dst)
    blocks = max(1, -(-covered // BLOCK)) + int(rng.integers(0, 3))      # the job may be longer than this input (another one is)
    # every output sample on its own: exactly the indices the formula reads, as a hull
    probe = sorted(set([0, 1, max(covered - 2, 0), max(covered - 1, 0), covered, covered + 1] + [int(v) for v in rng.integers(0, covered + 2, 50)]))
    for i in probe:
        first, count = pkg.batch_stream_span(n, src, dst, i, 1)
        if i >= covered:
            assert count == 0 and first == n, (n, src, dst, i)
            continue
        r = [i] if src == dst else reads(i, n, src, dst)
        assert (first, first + count) == (r[0], r[-1] + 1), (n, src, dst, i)
        assert first + count <= n
    # slices: the span of every slice, and the "new" part of it that need() would ask for
    brought, pos, total = 0, 0, 0
    for k in random_slicing(rng, blocks):
        first, count = pkg.batch_stream_span(n, src, dst, pos, k * BLOCK)
        want = want_span(n, src, dst, pos, k * BLOCK)
        if want is None:
            assert count == 0
        else:
            assert (first, first + count) == want, (n, src, dst, pos, k)
            assert 0 <= first and first + count <= n
            for i in [pos, min(pos + k * BLOCK, covered) - 1] + [int(v) for v in rng.integers(pos, min(pos + k * BLOCK, covered), 8)]:
                r = [i] if src == dst else reads(i, n, src, dst)
                assert first <= r[0] and r[-1] < first + count, (n, src, dst, pos, k, i)
            # what the slices before brought reaches back far enough: the window looks at most 6 frames behind the frames handed over
            assert first >= brought - 6, (n, src, dst, pos, first, brought)
            new_first, new_end = brought, max(brought, first + count)      # contiguous with the slice before, never twice
            assert new_first <= new_end <= n
            total += new_end - new_first
            brought = new_end
        pos += k * BLOCK
    assert total == brought <= n
    if src == dst:
        assert brought == n                                                # same rate: every frame, the identity cut at the file's end


def test_same_rate_is_the_identity_cut_at_the_end(pkg):
    assert pkg.batch_stream_span(20000, 48000, 48000, 0, BLOCK) == (0, BLOCK)
    assert pkg.batch_stream_span(20000, 48000, 48000, 2 * BLOCK, BLOCK) == (2 * BLOCK, 20000 - 2 * BLOCK)
    assert pkg.batch_stream_span(20000, 48000, 48000, 3 * BLOCK, BLOCK) == (20000, 0)
    assert pkg.batch_stream_span(0, 48000, 48000, 0, BLOCK) == (0, 0)


def test_positions_beyond_two_to_the_31_follow_python_integers(pkg):
    rng = np.random.default_rng(77)
    for _ in range(200):
        src, dst = int(rng.choice(RATES)), int(rng.choice(RATES[:5]))
        n = int(rng.integers(2 ** 33, 2 ** 36))
        covered = n if src == dst else out_length(n, src, dst)
        first_out = int(rng.integers(2 ** 31, covered - 1))
        count_out = int(rng.choice([1, BLOCK, 64 * BLOCK, 2 ** 31 - BLOCK, 2 ** 33]))
        first, count = pkg.batch_stream_span(n, src, dst, first_out, count_out)
        assert (first, first + count) == want_span(n, src, dst, first_out, count_out), (n, src, dst, first_out, count_out)
    # the file's very end
    n, src, dst = 2 ** 34 + 12345, 44100, 192000
    covered = out_length(n, src, dst)
    first, count = pkg.batch_stream_span(n, src, dst, covered - 5, 100)
    assert first + count == n and first == reads(covered - 5, n, src, dst)[0]
    assert pkg.batch_stream_span(n, src, dst, covered, 100) == (n, 0)


def test_span_rejects_what_it_should(pkg):
    with pytest.raises(pkg.GdgError):
        pkg.batch_stream_span(100, 0, 48000, 0, 10)
    with pytest.raises(pkg.GdgError):
        pkg.batch_stream_span(100, 48000, 0, 0, 10)
