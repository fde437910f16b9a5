"""The transfer records without a GPU: the section's layout, the list's validation and the planner as a stand-alone program
(tests/native/transfer_plan_check.cpp); the planner through the library -- its known answers against the numpy restatement
(tests/transfer_ref.py), its refusals, the ridge; gdg_transfer_doubles; every layer's names; and the compiler's resource summary of the
record kernel: no scratch, the LDS bytes of DESIGN.md's table."""
import os
import re
import subprocess

import numpy as np
import pytest

import transfer_ref as ref
import __graft_entry__ as entry
import list_chain_pins

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
NEW = ["gdg_batch_transfer_enable", "gdg_batch_transfers", "gdg_batch_transfer", "gdg_block_transfer_rows", "gdg_block_transfer_rows_device", "gdg_transfer_doubles",
       "gdg_match_taps_from_transfer"]
# The C planner and np.fft.irfft are two float64 inverse transforms of up to 8192 points in different butterfly orders.  Measured over D in
# {1, 8, 64}, seeds 1 to 8 of random H, n_taps = N' / 2, center 0 and 5: the largest |tap - ref| / max |ref| is 6.6e-15; with
# the margin of 4 for the different transform order:
PLAN_TOL = 4 * 6.6e-15


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def test_the_symbols_exist(pkg):
    for name in NEW:
        assert getattr(pkg.lib(), name) is not None and name in pkg.ABI_SYMBOLS
    for name in ("batch_transfer_enable", "batch_transfers", "batch_transfer", "block_transfer", "block_transfer_device", "transfer_doubles", "match_taps_from_transfer"):
        assert callable(getattr(pkg.Context, name)), name


def test_section_list_and_planner_as_a_stand_alone_program(tmp_path):
    exe = str(tmp_path / "transfer_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "native", "transfer_plan_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"OK transfer section, list and planner; (\d+) section cases, (\d+) moved by the 16-byte step\n", r.stdout)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) == 16 * 3 * 3 and int(m.group(2)) > 0                  # 16 on/off combinations x 3 widths x 3 ends


def test_the_section_rides_behind_the_three_kinds_and_the_kernel_is_part_of_fir_o():
    with open(os.path.join(CSRC, "report_sections.h")) as f:
        text = f.read()
    list_chain_pins.assert_one_chain(CSRC)                                      # the fourth entry of the one chain, behind the three kinds
    assert "static inline size_t transfer_record_bytes(size_t pairs, size_t group) { return pairs && group ? pairs * (4096 / group + 1) * 4 * 8 : 0; }" in text
    with open(os.path.join(CSRC, "ctx.h")) as f:
        assert "BATCH_TRANSFER_TABLE == BATCH_FIT_TABLE + LIST_TRANSFER" in f.read()       # its table's slot is the kind's
    with open(os.path.join(CSRC, "Makefile")) as f:
        make = f.read()
    assert "transfer_kernels.h" in [w for line in make.splitlines() if line.startswith("fir.o:") for w in line.split()]
    with open(os.path.join(CSRC, "fir.hip")) as f:
        fir = f.read()
    assert fir.index('#include "align_kernels.h"') < fir.index('#include "transfer_kernels.h"') < fir.index("#pragma clang fp contract(fast)")


def test_planner_known_answers(pkg):
    for D in (1, 8, 64):
        rec = ref.synth_records([1.0, -2.0, 3.0], D)
        for center in (0, 5):
            taps, coh = pkg.match_taps_from_transfer(rec, 1, D, 16, center)
            want = np.zeros(16)
            want[center:center + 3] = [1.0, -2.0, 3.0]
            want *= ref.taper(16, center)
            assert np.abs(taps[0] - want).max() <= PLAN_TOL * 3.0 and abs(coh[0] - 1.0) <= PLAN_TOL, (D, center, taps[0], coh)
            assert taps[0][center] == pytest.approx(1.0, abs=PLAN_TOL * 3.0) and (ref.taper(16, center) > 0.0).all()


def test_planner_against_the_numpy_restatement(pkg):
    worst = 0.0
    for D in (1, 8, 64):
        G = ref.groups(D)
        for seed in range(1, 9):
            rng = np.random.default_rng(seed)
            rec = np.zeros((2, 1, G, 4))
            rec[..., 0], rec[..., 1] = rng.uniform(0.5, 2.0, (2, 1, G)), rng.uniform(0.5, 2.0, (2, 1, G))
            rec[..., 2:] = rng.normal(size=(2, 1, G, 2))
            for center in (0, 5):
                taps, coh = pkg.match_taps_from_transfer(rec, 1, D, G - 1, center)
                want, want_coh = ref.plan(rec, 1, D, G - 1, center)
                worst = max(worst, np.abs(taps - want).max() / np.abs(want).max(), abs(coh[0] - want_coh[0]) / want_coh[0])
    print("planner against irfft: worst relative deviation %.3g" % worst)
    assert worst <= PLAN_TOL


def test_planner_refusals_write_nothing(pkg):
    rec = ref.synth_records([1.0, -2.0, 3.0], 8)
    lib = pkg.lib()
    tap, coh = np.full(16, 99.0), np.full(1, 99.0)

    def refused(r, D, n_taps, center, what, ridge=0.0):
        r = np.ascontiguousarray(r, dtype=np.float64)
        rc = lib.gdg_match_taps_from_transfer(r.ctypes.data, 1, D, r.shape[0], ridge, n_taps, center, tap.ctypes.data, coh.ctypes.data)
        assert rc == pkg.GDG_ERR_INVALID and re.search(what, lib.gdg_last_error(None).decode()), (rc, lib.gdg_last_error(None))
        assert (tap == 99.0).all() and coh[0] == 99.0, what

    bad = rec.copy()
    bad[0, 0, 3, 2] = np.nan
    refused(bad, 8, 16, 0, "pair 0: the summed record has a NaN or inf entry")
    silent = rec.copy()
    silent[..., 0] = 0.0
    refused(silent, 8, 16, 0, "pair 0: the summed record has no energy in the port")
    refused(rec, 8, 4096 // 8 + 1, 0, "n_taps = 513")
    refused(rec, 8, 16, 16, "center = 16")
    refused(rec, 3, 16, 0, "group = 3")
    refused(rec, 8, 16, 0, "ridge = -1", ridge=-1.0)
    with pytest.raises(pkg.GdgError, match="pair 0: the summed record has no energy"):
        pkg.match_taps_from_transfer(silent, 1, 8, 16)


def test_a_ridge_shrinks_every_gain_and_the_taps_energy(pkg):
    rng = np.random.default_rng(3)
    G = ref.groups(32)
    rec = np.zeros((3, 1, G, 4))
    rec[..., 0], rec[..., 1] = rng.uniform(0.1, 2.0, (3, 1, G)), rng.uniform(0.5, 2.0, (3, 1, G))
    rec[..., 2:] = rng.normal(size=(3, 1, G, 2))
    s = rec.sum(axis=0)[0]
    gain = lambda ridge: np.hypot(s[:, 2], s[:, 3]) / (s[:, 0] + ridge * s[:, 0].mean())
    assert (gain(1e-2) < gain(0.0)).all()
    plain, _ = pkg.match_taps_from_transfer(rec, 1, 32, 128, 0, 0.0)
    loaded, _ = pkg.match_taps_from_transfer(rec, 1, 32, 128, 0, 1e-2)
    assert np.sum(loaded ** 2) < np.sum(plain ** 2)


def test_transfer_doubles(pkg):
    for D in ref.GROUPS:
        for n in (1, 3, 16):
            assert pkg.transfer_doubles(n, D) == n * (4096 // D + 1) * 4 == ref.doubles(n, D)
    assert pkg.transfer_doubles(1, 1) * 8 == 131104
    assert pkg.transfer_doubles(0, 1) == pkg.transfer_doubles(17, 1) == pkg.transfer_doubles(1, 3) == pkg.transfer_doubles(1, 128) == pkg.transfer_doubles(1, 0) == 0


def test_every_layer_knows_the_calls_and_prototypes_equal_exports(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in exported and name in pkg.ABI_SYMBOLS and re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
    assert {n for n in exported if n.startswith("gdg_") and "transfer" in n and "launch" not in n} == set(NEW)
    assert (pkg.TRANSFER_BLOCK, pkg.TRANSFER_MAX_PAIRS, pkg.TRANSFER_MAX_GROUP) == (8192, 16, 64)
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("There is no doubling of the inner bins", "every bin lies in exactly one group", "added over ascending k", "every entry that involves it is exactly +0.0",
                   "measured against its OWN total", "Sxx = 0.25/24, 0.25/6, 0.25/24 in groups 99, 100, 101", "Im Sxy[100] = -0.25/6", "PARSEVAL",
                   "GDG_ERR_UNSUPPORTED while a transfer list is in force", "never collect transfer records", "The coherence is 1 by construction for one block at D = 1",
                   "averaging over blocks or groups is what makes it a measurement", "nothing is written on a refusal", "radix-2 decimation-in-time"):
        assert phrase in flat, phrase
    for macro, value in (("GDG_TRANSFER_BLOCK", 8192), ("GDG_TRANSFER_MAX_PAIRS", 16), ("GDG_TRANSFER_MAX_GROUP", 64)):
        assert re.search(r"^#define %s %d$" % (macro, value), header, re.M)
    with open(os.path.join(os.path.dirname(os.path.dirname(pkg.LIB_PATH)), "go", "gdg", "gdg.go")) as f:
        go = f.read()
    for sig in (r"^func \(this \*Context\) BatchTransferEnable\(pairs \[\]TransferPair, group int\) error", r"^func \(this \*Context\) BatchTransfers\(\) int",
                r"^func \(this \*Context\) BatchTransfer\(\) \(\[\]\[\]float64, error\)", r"^func \(this \*Context\) BlockTransferRows\(", r"^func \(this \*Context\) BlockTransferRowsDevice\(",
                r"^func TransferDoubles\(nPairs int, group int\) int", r"^func MatchTapsFromTransfer\("):
        assert re.search(sig, go, re.M), sig
    for name in NEW:
        assert "C.%s(" % name in go, name


def design_table():
    """the resources table of DESIGN.md 4.12h: {row name: text}"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    part = text[text.index("### 4.12h"):]
    part = part[:part.index("\n## ")]
    assert "| | block_transfer_kernel |" in part
    return dict(re.findall(r"^\| ([^|]+?) \| ([^|]+?) \|$", part, re.M))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_transfer_kernel_uses_no_scratch_and_the_lds_of_the_table(tmp_path):
    """block_transfer_kernel (both load paths) from the compiler's resource summary of fir.hip: no scratch; LDS of two padded arrays of
    8192 + 512 + 16 doubles, 139 520 bytes, the figure DESIGN.md 4.12h states; at most 256 VGPRs (512 threads are two waves per SIMD)."""
    out = str(tmp_path / "fir.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "fir.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @(.*?)^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        if "block_transfer_kernel" in m.group(1):
            found[m.group(1)] = (int(m.group(3)), int(m.group(4)), int(m.group(5)))
    assert len(found) == 2, sorted(found)                                        # VEC and scalar: the kernel is part of fir.o's device code
    rows = design_table()
    stated = int(re.match(r"([\d ]+) bytes", rows["LDS of a workgroup"]).group(1).replace(" ", ""))
    stated_vgprs = {"ILb1E": int(re.search(r"(\d+) \(VEC\)", rows["VGPRs of a thread"]).group(1)), "ILb0E": int(re.search(r"(\d+) \(scalar\)", rows["VGPRs of a thread"]).group(1))}
    for name, (vgprs, scratch, lds) in found.items():
        assert scratch == 0 == int(rows["scratch bytes"]) and lds == 2 * (8192 + 512 + 16) * 8 == stated, (name, scratch, lds, stated)
        path = "ILb1E" if "ILb1E" in name else "ILb0E"
        assert vgprs == stated_vgprs[path] <= 256, (name, vgprs, stated_vgprs)       # both figures of the table, exactly
