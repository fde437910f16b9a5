"""The Gram list without a GPU: the Gram section's layout, the packed index and the greedy planner as a stand-alone program
(tests/native/gram_plan_check.cpp), built plainly and once more under AddressSanitizer and UBSan; the planner through the library against
numpy.linalg.lstsq at every step; its weights against the fit planner's, bit for bit; its refusals; the header as pedantic C99; every
layer's names; and the compiler's resource summary of the record kernel: no scratch, LDS for two workgroups per CU, the FP64 matrix
instruction."""
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import list_chain_pins

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
NEW = ["gdg_batch_gram_enable", "gdg_batch_gram_ports", "gdg_batch_gram", "gdg_block_gram_rows", "gdg_block_gram_rows_device", "gdg_blend_pick_from_gram"]

C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gdg.h"
int main(void) {
    const int port[2] = { 0, 1 }, cand[1] = { 1 };
    double a[2] = { 1.0, 2.0 }, b[2] = { 3.0, 4.0 }, rec[3] = { 4.0, 2.0, 4.0 }, w[8], res[8];
    const double *rows[2];
    int picked[8], n = 7, got[2];
    size_t blocks = 7;
    rows[0] = a; rows[1] = b;
    printf("%d %d %d %d %d\n", gdg_batch_gram_enable(NULL, port, 2), gdg_batch_gram_ports(NULL, got, 2), gdg_batch_gram(NULL, rec, 3, &blocks),
           gdg_block_gram_rows(NULL, rows, 2, 2, 2, port, 2, rec), gdg_block_gram_rows_device(NULL, a, 2, 2, 2, 2, port, 2, rec));
    got[0] = gdg_blend_pick_from_gram(rec, 2, 1, 0, cand, 1, 1, 0.0, 0.0, picked, w, res, &n);
    printf("%d %d %d %g %g\n", got[0], n, picked[0], w[0], res[0]);
    printf("%d\n", GDG_GRAM_MAX_PORTS);
    return 0;
}
"""


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_gram_section_index_and_planner_as_a_stand_alone_program(tmp_path, flags):
    exe = str(tmp_path / "gram_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "gram_plan_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"OK gram section, index and picks; (\d+) section cases, (\d+) moved by the 16-byte step\n", r.stdout)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) == 6 * 6 * 4 and int(m.group(2)) > 0                 # 6 ends x 6 port counts x 4 step widths


def test_the_gram_section_is_stated_once_and_is_no_fifth_kind():
    with open(os.path.join(CSRC, "report_sections.h")) as f:
        text = f.read()
    assert "enum { REPORT_STATS, REPORT_BANDS, REPORT_ALIGN, REPORT_TRUE_PEAK, REPORT_KINDS };" in text
    list_chain_pins.assert_one_chain(CSRC)                                      # a list record of its own: one enum, one chain, one store array
    assert "static inline size_t gram_record_bytes(size_t ports) { return ports * (ports + 1) / 2 * 8; }" in text
    with open(os.path.join(CSRC, "Makefile")) as f:
        make = f.read()
    assert "gram_kernels.h" in [w for line in make.splitlines() if line.startswith("gram.o:") for w in line.split()]
    assert "gram.o" in [w for line in make.splitlines() if line.startswith("OBJS") for w in line.split()]


def packed(G):
    return G[np.tril_indices(G.shape[0])][None, :].copy()


def lstsq_share(x, t, chosen):
    """the share of t's energy that the least-squares blend of the rows `chosen` leaves"""
    A = x[chosen].T
    w = np.linalg.lstsq(A, t, rcond=None)[0]
    r = t - A @ w
    return float(r @ r) / float(t @ t)


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_planner_picks_what_lstsq_picks_at_every_step(pkg, seed):
    """12 random candidate rows and a target of 4096 samples, the Gram made with numpy.  At every step the pick is the arg-min over the
    candidates of lstsq's residual for the extended set; the runner-up lies at least 1e-6 of T behind (asserted here, on the numpy side),
    so that no rounding difference -- about 1e-13 of T in either computation -- decides a pick."""
    rng = np.random.default_rng(seed)
    L, P = 4096, 12
    x = rng.normal(size=(P, L)) + 0.4 * rng.normal(size=(1, L))
    t = rng.uniform(-1, 1, P) * (rng.uniform(size=P) < 0.5) @ x + 0.2 * rng.normal(size=L)
    X = np.vstack([t[None, :], x])
    rec = packed(X @ X.T)
    T = float(t @ t)
    for max_terms in (1, 2, 3, 4):
        picked, weights, residuals = pkg.blend_pick_from_gram(rec, P + 1, 0, range(1, P + 1), max_terms)
        assert len(picked) == max_terms
        chosen = []
        for m in range(max_terms):
            shares = sorted((lstsq_share(x, t, chosen + [c]), c) for c in range(P) if c not in chosen)
            assert shares[1][0] - shares[0][0] >= 1e-6, (seed, m, shares[:2])
            assert picked[m] - 1 == shares[0][1], (seed, max_terms, m, picked, shares[:2])
            chosen.append(shares[0][1])
            assert abs(residuals[m] - shares[0][0]) <= 1e-10, (residuals[m], shares[0][0])
        want = np.linalg.lstsq(x[chosen].T, t, rcond=None)[0]
        assert np.abs(weights - want).max() <= 1e-10 * np.abs(want).max()
    assert T > 0


@pytest.mark.parametrize("ridge", [0.0, 0.02])
def test_planner_weights_are_the_fit_planner_s_bit_for_bit(pkg, ridge):
    rng = np.random.default_rng(77)
    P, blocks = 9, 3
    X = rng.normal(size=(P + 1, blocks, 512)) + 0.5 * rng.normal(size=(1, blocks, 512))
    rec = np.concatenate([packed(X[:, q] @ X[:, q].T) for q in range(blocks)], axis=0)
    picked, weights, residuals = pkg.blend_pick_from_gram(rec, P + 1, 0, range(1, P + 1), 4, ridge)
    assert len(picked) == 4
    fit = np.zeros((1, blocks), dtype=pkg.FIT_DTYPE)
    for q in range(blocks):
        fit[0, q]["terms"] = 4
        fit[0, q]["tt"] = rec[q, pkg.gram_index(0, 0)]
        for j, a in enumerate(picked):
            fit[0, q]["tx"][j] = rec[q, pkg.gram_index(a, 0)]
            for k, b in enumerate(picked[:j + 1]):
                fit[0, q]["xx"][j * (j + 1) // 2 + k] = rec[q, pkg.gram_index(a, b)]
    w, res = pkg.blend_weights_from_fit(fit, ridge)
    assert w[0, :4].tobytes() == weights.tobytes() and not w[0, 4:].any()
    assert res[0].tobytes() == residuals[3].tobytes()


def test_planner_refusals_reach_the_caller_and_a_duplicate_is_skipped(pkg):
    rng = np.random.default_rng(5)
    x = rng.normal(size=(4, 256))
    t = 0.5 * x[1] + 0.25 * x[3]
    X = np.vstack([t[None], x, x[1][None]])                                      # position 5 duplicates position 2
    G = X @ X.T
    picked, weights, residuals = pkg.blend_pick_from_gram(packed(G), 6, 0, [5, 1, 2, 3, 4], 3, min_gain=1e-9)
    assert picked == [5, 4] and np.abs(weights - [0.5, 0.25]).max() <= 1e-12 and residuals[1] <= 1e-12      # the duplicate (2) is skipped, the other one is picked; then nothing gains
    picked, _, _ = pkg.blend_pick_from_gram(packed(G), 6, 0, [1, 2, 3, 4, 5], 3, min_gain=1e-9)
    assert picked == [2, 4]
    Z = G.copy()
    Z[0, 0] = 0.0
    with pytest.raises(pkg.GdgError, match="the target .list position 0. is silent") as e:
        pkg.blend_pick_from_gram(packed(Z), 6, 0, [1, 2, 3], 2)
    assert e.value.code == pkg.GDG_ERR_INVALID
    N = G.copy()
    N[3, 1] = N[1, 3] = np.nan
    with pytest.raises(pkg.GdgError, match="NaN or inf entry at list position 1"):
        pkg.blend_pick_from_gram(packed(N), 6, 0, [1, 2, 3], 2)
    with pytest.raises(pkg.GdgError, match="candidate 2 is list position 1, which is the target or an earlier candidate"):
        pkg.blend_pick_from_gram(packed(G), 6, 0, [1, 2, 1], 2)
    with pytest.raises(pkg.GdgError, match=r"max_terms = 9 \(1 to 8\)"):
        pkg.blend_pick_from_gram(packed(G), 6, 0, [1, 2, 3], 9)


def test_the_header_is_pedantic_c99_with_the_gram_calls(pkg, tmp_path):
    src = tmp_path / "gram_probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "gram_probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    inv = pkg.GDG_ERR_INVALID
    assert [int(v) for v in lines[0].split()] == [inv, 0, inv, inv, inv]             # no context: refused, nothing touched; no list in force
    assert lines[1] == "0 1 1 0.5 0.75" and lines[2] == "512"                        # G = [[4, 2], [2, 4]]: w = 2 / 4, and 4 - 2 + 1 = 3 of 4 are left


def test_every_layer_knows_the_calls(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in exported and name in pkg.ABI_SYMBOLS and re.search(r"^int %s\(" % name, header, re.M), name
    for name in ("batch_gram_enable", "batch_gram_ports", "batch_gram", "block_gram", "block_gram_device"):
        assert callable(getattr(pkg.Context, name)), name
    assert callable(pkg.blend_pick_from_gram) and pkg.GRAM_MAX_PORTS == 512
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("one accumulator chain of that instruction, started at +0.0, over k = 0, 4, 8, ... ascending", "Samples behind the block's end count as +0.0",
                   "is never split over k across waves or workgroups, uses no atomics and is never finished by a second pass",
                   "The entry is NOT bit for bit the sum_sq of gdg_block_stats", "GDG_ERR_UNSUPPORTED while a Gram list is in force", "never collect Gram records",
                   "at P = 512 a record is 1 050 624 bytes", "is skipped, not refused"):
        assert phrase in flat, phrase
    assert re.search(r"^#define GDG_GRAM_MAX_PORTS 512$", header, re.M)
    with open(os.path.join(os.path.dirname(os.path.dirname(pkg.LIB_PATH)), "go", "gdg", "gdg.go")) as f:
        go = f.read()
    for sig in (r"^func \(this \*Context\) BatchGramEnable\(ports \[\]int\) error", r"^func \(this \*Context\) BatchGramPorts\(\) \[\]int",
                r"^func \(this \*Context\) BatchGram\(\) \(\[\]\[\]float64, error\)", r"^func \(this \*Context\) BlockGramRows\(", r"^func \(this \*Context\) BlockGramRowsDevice\(",
                r"^func BlendPickFromGram\(records \[\]\[\]float64, nPorts int, target int, candidates \[\]int, maxTerms int, ridge float64, minGain float64\)"):
        assert re.search(sig, go, re.M), sig
    for call in ("C.gdg_batch_gram_enable(", "C.gdg_batch_gram_ports(", "C.gdg_batch_gram(", "C.gdg_block_gram_rows(", "C.gdg_block_gram_rows_device(", "C.gdg_blend_pick_from_gram("):
        assert call in go, call
    from go_dsp_guitar_amd import host
    assert callable(host.Engine._set_gram) and callable(host.Engine.render_matched) and host.lib().gdgh_engine_set_batch_gram is not None
    assert host.lib().gdgh_engine_last_batch_gram is not None
    with open(os.path.join(os.path.dirname(os.path.dirname(pkg.LIB_PATH)), "host", "gdg_host.hpp")) as f:
        hpp = f.read()
    assert "Error SetBatchGram(const std::vector<int> &ports);" in hpp
    assert "Error LastBatchGram(std::vector<double> &records, int *ports, size_t *blocks) const;" in hpp
    assert os.path.exists(os.path.join(ROOT, "profiles", "probes", "batch_gram.py"))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_gram_kernel_uses_no_scratch_little_lds_and_the_f64_matrix_instruction(tmp_path):
    """block_gram_kernel from the compiler's resource summary: no scratch; LDS of two 64-row panels of 34 doubles, 34816 bytes -- far below
    the 80 KiB that let two workgroups share a CU --; and its instruction stream holds v_mfma_f64_16x16x4_f64, 4 accumulators x 8 steps of
    k per chunk."""
    out = str(tmp_path / "gram.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "gram.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @(.*?)^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        if "block_gram_kernel" in m.group(1):
            found[m.group(1)] = (int(m.group(3)), int(m.group(4)), int(m.group(5)), m.group(2).count("v_mfma_f64_16x16x4"))
    assert len(found) == 1, sorted(found)
    for name, (vgprs, scratch, lds, mfma) in found.items():
        assert scratch == 0 and lds == 2 * 64 * 34 * 8 and lds <= 80 * 1024 and vgprs <= 256, (name, vgprs, scratch, lds)
        assert mfma >= 4 and mfma % 4 == 0, (name, mfma)
