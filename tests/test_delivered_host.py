"""The delivered rows' records (include/gdg.h, DELIVERED RECORDS) without a GPU: the numpy restatement (tests/delivered_ref.py) against the
definition's known answers and its own rules -- a stream cut anywhere and carried through the history gives the records of the one call; the
samples' part against plain numpy -- and the block spans as a program of its own (tests/native/delivered_spans_check.cpp), once more under
the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np

import __graft_entry__ as entry
import delivered_ref as ref
import true_peak_ref

ROOT = entry.ROOT
CSRC = os.path.join(entry.PKG_DIR, "csrc")
TAPS = true_peak_ref.formula_taps()


def test_known_answers():
    o = 1882
    span = [0, o, 2 * o, 3 * o]
    silent = ref.block_delivered(np.zeros(3 * o), span, TAPS)
    assert silent.tobytes() == bytes(silent.nbytes)
    x = np.zeros(3 * o)
    x[o + 100] = 1.0
    rec = ref.block_delivered(x, span, TAPS)[0]
    assert (rec[1]["true_peak"], rec[1]["position"], rec[1]["overs"], rec[1]["peak"], rec[1]["peak_index"], rec[1]["sum_sq"]) == (1.0, 400, 0, 1.0, 100, 1.0)
    assert rec[0].tobytes() == bytes(40) and rec[2].tobytes() == bytes(40)
    x = np.zeros(3 * o)
    x[o - 1] = x[o] = 0.8
    rec = ref.block_delivered(x, span, TAPS)[0]
    assert abs(TAPS[1, 11] - 0.633825) < 1e-6 and TAPS[1, 11] == TAPS[1, 12]
    assert rec[1]["peak"] == 0.8 and rec[1]["true_peak"] == 0.8 * TAPS[1, 11] + 0.8 * TAPS[1, 12] and abs(rec[1]["true_peak"] - 1.0141) < 1e-4
    assert (rec[1]["position"], rec[1]["overs"], rec[1]["peak_index"], rec[1]["clipped"]) == (-2, 1, 0, 0)
    assert (rec[0]["true_peak"], rec[0]["peak"], rec[0]["position"], rec[0]["overs"]) == (0.8, 0.8, 4 * (o - 1), 0)
    # the hole: the stateless true-peak record of either block alone sees 0.8
    for part in (x[:o], x[o:2 * o]):
        alone = true_peak_ref.block_true_peak([part], TAPS)[0, 0]
        assert alone["true_peak"] == 0.8 and alone["overs"] == 0
    # the lowest position: a block of one sample whose largest point is the first of the interval twelve in front of it
    x = np.zeros(40)
    x[0] = 1.0                                                               # in the lead-in of the block [23, 24): read by tap 0 of interval 11 alone
    rec = ref.block_delivered(x, [0, 23, 24, 40], TAPS)[0, 1]
    assert rec["peak"] == 0.0 and rec["position"] in (-47, -46, -45) and rec["true_peak"] == np.abs(TAPS[:, 0]).max()


def test_a_stream_cut_anywhere_is_the_stream_in_one_call():
    rng = np.random.default_rng(3)
    x = rng.uniform(-1.1, 1.1, (2, 6000))
    x[0, 77] = np.nan
    x[1, 4095] = np.inf
    span = [0, 1, 24, 1905, 3787, 4096, 6000]
    whole = ref.block_delivered(x, span, TAPS)
    assert whole["overs"].sum() > 0 and whole["clipped"].sum() > 0
    for k in (1, 2, 4):                                                      # a first call of one sample, of 24, and one that ends behind the inf
        cut = span[k]
        hist = np.zeros((2, ref.HISTORY))
        a = ref.block_delivered(x[:, :cut], span[:k + 1], TAPS, hist)
        b = ref.block_delivered(x[:, cut:], [s - cut for s in span[k:]], TAPS, hist)
        assert np.concatenate([a, b], axis=1).tobytes() == whole.tobytes(), cut
        assert np.array_equal(hist, x[:, -ref.HISTORY:])
    # the samples' part is plain: the first largest magnitude, the count above 1, and a sum of squares within the order's rounding
    clean = ref.finite(x)
    for r in range(2):
        for k in range(len(span) - 1):
            blk = clean[r, span[k]:span[k + 1]]
            rec = whole[r, k]
            assert rec["peak"] == np.abs(blk).max() and rec["peak_index"] == int(np.argmax(np.abs(blk))) and rec["clipped"] == np.count_nonzero(np.abs(blk) > 1.0)
            assert abs(rec["sum_sq"] - float(np.sum(blk * blk))) <= 1e-12 * max(1.0, float(np.sum(blk * blk)))
            assert rec["true_peak"] >= rec["peak"]


def test_the_block_spans_as_a_stand_alone_program(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "delivered_spans_check.cpp")
    for name, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("delivered_spans_check_" + name))
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, src, "-o", exe], check=True, timeout=300)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        m = re.match(r"OK delivered block spans; (\d+) step cases\n", r.stdout)
        assert m and int(m.group(1)) > 1000, r.stdout + r.stderr
