"""The loudness records (include/gdg.h, LOUDNESS) without a GPU: the known answers of BS.1770 and EBU Tech 3341 (their own tolerance is
0.1 LU) from the sequential restatement's hop sums through the library's planner; the hop count; the coefficients against the standard's
table; the trim planner's cap; and the planners as a stand-alone program (tests/native/loudness_check.cpp), built plainly and once more
under AddressSanitizer and UBSan."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import loudness_ref as ref

ROOT = entry.ROOT
CSRC = os.path.join(entry.PKG_DIR, "csrc")


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def sine(freq, dbfs, seconds, rate):
    return 10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * freq * np.arange(int(seconds * rate)) / rate)


@pytest.mark.parametrize("rate", [44100, 48000, 192000])
def test_a_full_scale_997_hz_sine_reads_minus_3_01(pkg, rate):
    rec = ref.hop_sums(ref.k_weight(sine(997.0, 0.0, 2.0, rate), rate), rate)[None, :]
    got = pkg.loudness_from_hops(rec, rate, [0])
    want = ref.from_hops(rec, rate, [0])
    print(rate, got)
    assert abs(got[0] + 3.01) <= 0.1 and abs(got[1] + 3.01) <= 0.1 and got[2] == -math.inf      # 2 s: no 3 s window
    assert all(abs(a - b) < 1e-9 for a, b in zip(got[:2], want[:2]))


def test_a_stereo_1_khz_sine_at_minus_23_dbfs_reads_minus_23(pkg):
    rate = 48000
    one = ref.hop_sums(ref.k_weight(sine(1000.0, -23.0, 4.0, rate), rate), rate)
    rec = np.stack([one, one, np.zeros_like(one)])
    got = pkg.loudness_from_hops(rec, rate, [0, 1], [1.0, 1.0])
    print(got)
    assert all(abs(v + 23.0) <= 0.1 for v in got)
    assert pkg.loudness_from_hops(rec, rate, [2])[0] == -math.inf               # silence reads -inf, and succeeds
    assert abs(pkg.loudness_from_hops(rec, rate, [0, 1, 2], [1.0, 1.0, 1.41])[0] - got[0]) < 1e-12


def test_the_gating_sequence_reads_minus_23(pkg):
    """-36 dBFS for 10 s, -23 dBFS for 60 s, -36 dBFS for 10 s on both channels: the relative gate drops the quiet parts"""
    rate = 48000
    x = np.concatenate([sine(1000.0, -36.0, 10.0, rate), sine(1000.0, -23.0, 60.0, rate), sine(1000.0, -36.0, 10.0, rate)])
    one = ref.hop_sums(ref.k_weight(x, rate), rate)
    rec = np.stack([one, one])
    got = pkg.loudness_from_hops(rec, rate, [0, 1])
    ungated = ref.lufs(2.0 * one.sum() / (one.size * (rate // 10)))
    print(got, "ungated", ungated)
    assert rec.shape == (2, 800) and abs(got[0] + 23.0) <= 0.1 and ungated < -23.3
    assert abs(got[0] - ref.from_hops(rec, rate, [0, 1])[0]) < 1e-9


def test_the_hop_count_is_the_plain_integer_formula(pkg):
    for rate in (44100, 48000):
        h = rate // 10
        for first in range(0, 2 * h, 211):
            for count in range(0, h + 400, 53):
                assert pkg.loudness_hops(rate, first, count) == sum(1 for k in range(4) if first < (k + 1) * h <= first + count), (rate, first, count)
    assert pkg.loudness_hops(44101, 0, 10 ** 6) == 0


def test_the_coefficients_are_the_standards_table_and_design_md_says_how_close(pkg):
    got = pkg.loudness_coefficients(48000)
    worst = float(np.max(np.abs(got - np.array(ref.BS1770_48K))))
    print("largest difference from the BS.1770 table: %.3e" % worst)
    assert worst < 5e-14                                                     # the table is printed to 14 decimals
    assert np.array_equal(got, np.array(ref.coefficients(48000)))
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        part = f.read().split("### 4.12l")[1]
    m = re.search(r"largest difference from the table printed in BS\.1770 is ([0-9.e-]+)", part)
    assert m and float(m.group(1)) >= worst and float(m.group(1)) < 1e-13
    for rate in (44100, 96000, 192000):
        assert np.array_equal(pkg.loudness_coefficients(rate), np.array(ref.coefficients(rate))), rate
    with pytest.raises(pkg.GdgError, match="loudness coefficients: rate 44101"):
        pkg.loudness_coefficients(44101)


def test_the_trim_planner_and_its_cap(pkg):
    rate, hops = 48000, 60
    rec = np.zeros((3, hops))
    rec[0] = 4800.0 * 10.0 ** (-30.0 / 10.0)                                  # reads -30.691 LUFS
    rec[1] = 4800.0 * 10.0 ** (-10.0 / 10.0)
    tp = np.zeros((3, 4), dtype=pkg.BLOCK_TRUE_PEAK_DTYPE)
    tp["true_peak"][0] = 0.9                                                 # +7.691 dB would carry it to 2.18: capped at -1 dBTP
    tp["true_peak"][1] = 0.5
    gain, capped = pkg.trim_from_loudness(rec, rate, -23.0, -1.0, tp)
    want, want_capped = ref.trim_from_loudness(rec, rate, -23.0, -1.0, tp["true_peak"])
    assert list(capped) == [True, False, False] == list(want_capped) and np.allclose(gain, want, rtol=1e-12, atol=0)
    assert gain[0] == 10.0 ** (-1.0 / 20.0) / 0.9 and abs(20 * math.log10(gain[1]) - (-23.0 + 10.691)) < 1e-9 and gain[2] == 1.0
    free, none = pkg.trim_from_loudness(rec, rate, -23.0)
    assert not none.any() and abs(20 * math.log10(free[0]) - 7.691) < 1e-9
    with pytest.raises(pkg.GdgError, match="trim from loudness: target_lufs"):
        pkg.trim_from_loudness(rec, rate, math.nan)
    bad = rec.copy()
    bad[1, 5] = -1.0
    with pytest.raises(pkg.GdgError, match="hop record 65 is negative"):
        pkg.trim_from_loudness(bad, rate, -23.0)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_the_planners_as_a_stand_alone_program(tmp_path, flags):
    exe = str(tmp_path / "loudness_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "loudness_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.match(r"OK loudness planners; \d+ cases; coefficients within \S+ of the BS\.1770 table\n", r.stdout), r.stdout + r.stderr
    assert not r.stderr, r.stderr                                            # a sanitizer's report
