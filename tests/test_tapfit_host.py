"""The tap fit without a GPU: the planner, the list's validation and the section's layout as a stand-alone program
(tests/native/tapfit_plan_check.cpp), built plainly and once more under AddressSanitizer and UBSan; the planner through the library -- its
known answers, its refusals, its bits against the fit planner's for up to 8 unknowns and against the numpy restatement; gdg_tapfit_doubles;
the header as pedantic C99 with the new calls; every layer's names; and the compiler's resource summary of the record kernel: no scratch,
the LDS bytes of DESIGN.md's table, the FP64 matrix instruction."""
import os
import re
import subprocess

import numpy as np
import pytest

import tapfit_ref as ref
import __graft_entry__ as entry
import list_chain_pins

ROOT = entry.ROOT
CSRC = os.path.join(ROOT, "go-dsp-guitar_amd", "csrc")
NEW = ["gdg_batch_tapfit_enable", "gdg_batch_tapfits", "gdg_batch_tapfit", "gdg_block_tapfit_rows", "gdg_block_tapfit_rows_device", "gdg_tapfit_doubles",
       "gdg_blend_taps_from_tapfit"]

C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gdg.h"
int main(void) {
    const int first[2] = { 0, 1 }, port[1] = { 0 }, target[1] = { 1 }, taps[1] = { 1 };
    double a[2] = { 1.0, 2.0 }, b[2] = { 3.0, 4.0 }, rec[3] = { 4.0, 2.0, 3.0 }, h[1], res[1];
    const double *rows[2];
    size_t blocks = 7, per = 7;
    int rc;
    rows[0] = a; rows[1] = b;
    printf("%d %d %d %d %d\n", gdg_batch_tapfit_enable(NULL, 1, first, port, target, taps), gdg_batch_tapfits(NULL), gdg_batch_tapfit(NULL, rec, 3, &blocks, &per),
           gdg_block_tapfit_rows(NULL, rows, 2, 2, 2, 1, first, port, target, taps, rec), gdg_block_tapfit_rows_device(NULL, a, 2, 2, 2, 2, 1, first, port, target, taps, rec));
    rc = gdg_blend_taps_from_tapfit(rec, 1, first, taps, 1, 0.0, h, res);
    printf("%d %g %d\n", rc, h[0], (int)gdg_tapfit_doubles(1, first, taps));
    printf("%d %d %d\n", GDG_TAPFIT_MAX_TERMS, GDG_TAPFIT_MAX_UNKNOWNS, GDG_TAPFIT_MAX_FITS);
    return 0;
}
"""


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_planner_list_and_section_as_a_stand_alone_program(tmp_path, flags):
    exe = str(tmp_path / "tapfit_plan_check")
    subprocess.run(["g++", "-std=c++17", "-Wall"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "native", "tapfit_plan_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"OK tap-fit planner, list and section; (\d+) section cases, (\d+) moved by the 16-byte step\n", r.stdout)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) == 5 * 4 * 3 and int(m.group(2)) > 0                 # 5 ends x 4 record sizes x 3 step widths


def test_the_section_is_stated_once_and_the_kernel_is_part_of_gram_o():
    with open(os.path.join(CSRC, "report_sections.h")) as f:
        text = f.read()
    assert "enum { REPORT_STATS, REPORT_BANDS, REPORT_ALIGN, REPORT_TRUE_PEAK, REPORT_KINDS };" in text
    list_chain_pins.assert_one_chain(CSRC)                                      # a list record of its own: one enum, one chain, one store array
    with open(os.path.join(CSRC, "Makefile")) as f:
        make = f.read()
    assert "tapfit_kernels.h" in [w for line in make.splitlines() if line.startswith("gram.o:") for w in line.split()]
    with open(os.path.join(CSRC, "gram.hip")) as f:
        assert '#include "tapfit_kernels.h"' in f.read()


def impulses(L=40):
    """four impulses of +-2 more than the taps apart and away from the ends: A = 16 I, so every root and quotient of the solve is exact"""
    x = np.zeros(L, dtype=np.int64)
    x[[5, 12, 20, 31]] = [2, -2, 2, 2]
    return x


def filtered(x, h):
    t = np.zeros_like(x)
    for a, v in enumerate(h):
        t[a:] += v * x[:x.size - a]
    return t


def test_planner_known_answers(pkg):
    h, res = pkg.blend_taps_from_tapfit(np.array([[4.0, 2.0, 3.0]]), [(1, [0], 1)])             # U = 1, A = 4, b = 2
    assert h[0].tolist() == [[0.5]] and abs(res[0] - 2.0 / 3.0) <= 1e-15
    # integer rows, the target filtered by the integer taps {1, -2, 3}: every sum is exact; to the last bit, and nothing is left
    x = impulses()
    rows = np.stack([x, filtered(x, [1, -2, 3])])
    fits = [(1, [0], 3)]
    rec = ref.record_int(rows, fits, 40)
    h, res = pkg.blend_taps_from_tapfit(rec, fits)
    assert h[0].tobytes() == np.array([[1.0, -2.0, 3.0]]).tobytes() and res[0] == 0.0 and not np.signbit(res[0])
    # random integer rows: the sums are still exact, the factorisation's roots are not -- within U 2^-52 cond(A) of the taps
    xr = np.random.default_rng(1).integers(-8, 9, 200)
    rows = np.stack([xr, filtered(xr, [1, -2, 3])])
    rec = ref.record_int(rows, fits, 100)
    h, res = pkg.blend_taps_from_tapfit(rec, fits)
    cond = np.linalg.cond(ref.unpack(rec.sum(axis=0), 1, 3)[:3, :3])
    assert np.max(np.abs(h[0] - [1.0, -2.0, 3.0])) <= 3 * 2.0 ** -52 * cond * 3.0 and res[0] <= 3 * 2.0 ** -52 * cond
    # the numpy restatement gives the library's bits
    (h_np, res_np), = ref.plan(rec, fits)
    assert h[0].tobytes() == h_np.tobytes() and res[0] == res_np


def test_one_port_twice_is_refused_and_named_without_a_ridge_and_gives_equal_taps_with_one(pkg):
    xr = np.random.default_rng(2).integers(-8, 9, 300)
    rows = np.stack([xr, filtered(xr, [1, -2, 3])])
    fits = [(1, [0], 3), (1, [0, 0], 2)]
    rec = ref.record_int(rows, fits, 300)
    with pytest.raises(pkg.GdgError, match="fit 1, term 1, lag 0: a pivot at or below") as e:
        pkg.blend_taps_from_tapfit(rec, fits)
    assert e.value.code == pkg.GDG_ERR_INVALID and "ridge" in str(e.value)
    ridge = 1e-3
    h, res = pkg.blend_taps_from_tapfit(rec, fits, ridge)
    # the two copies' difference lies along the direction the ridge alone holds: roundings of U 2^-52 grow by 1 / ridge
    assert np.max(np.abs(h[1][0] - h[1][1])) <= 4 * 2.0 ** -52 / ridge * np.max(np.abs(h[1])) and h[1].all()
    bad = rec.copy()
    bad[0, 4] = np.nan                                                           # entry (2, 1) of fit 0: term 0, lag 2
    with pytest.raises(pkg.GdgError, match="fit 0, term 0, lag 2: the summed record has a NaN or inf"):
        pkg.blend_taps_from_tapfit(bad, fits, ridge)
    with pytest.raises(pkg.GdgError, match="ridge = -1"):
        pkg.blend_taps_from_tapfit(rec, fits, -1.0)


@pytest.mark.parametrize("K,T", [(1, 1), (1, 5), (2, 4), (4, 2), (1, 8), (3, 2)])
def test_up_to_8_unknowns_the_taps_are_the_fit_planner_s_weights_bit_for_bit(pkg, K, T):
    U = K * T
    rng = np.random.default_rng(10 * K + T)
    rows = rng.normal(size=(K + 1, 2 * 600))
    fits = [(K, list(range(K)), T)]
    rec = np.stack([ref.packed(v @ v.T) for v in (ref.shifted_rows(rows, K, list(range(K)), T, b * 600, 600) for b in range(2))])
    fit_rec = np.zeros((1, 2), dtype=pkg.FIT_DTYPE)
    for q in range(2):
        G = ref.unpack(rec[q], K, T)
        fit_rec[0, q]["tt"], fit_rec[0, q]["terms"] = G[U, U], U
        fit_rec[0, q]["tx"][:U] = G[U, :U]
        fit_rec[0, q]["xx"][:U * (U + 1) // 2] = G[:U, :U][np.tril_indices(U)]
    for ridge in (0.0, 0.01):
        h, res = pkg.blend_taps_from_tapfit(rec, fits, ridge)
        w, wres = pkg.blend_weights_from_fit(fit_rec, ridge)
        assert h[0].reshape(-1).tobytes() == w[0, :U].tobytes() and res[0] == wres[0], (K, T, ridge)


def test_tapfit_doubles(pkg):
    assert pkg.tapfit_doubles([(0, [1], 1)]) == 3 and pkg.tapfit_doubles([(0, [1, 2], 64)]) == 129 * 130 // 2
    assert pkg.tapfit_doubles([(0, [1], 64), (0, [1, 2, 3, 0], 5), (9, [9], 7)]) == 65 * 66 // 2 + 21 * 22 // 2 + 8 * 9 // 2 == ref.list_doubles([(0, [1], 64), (0, [1, 2, 3, 0], 5), (9, [9], 7)])
    assert pkg.tapfit_doubles([]) == 0


def test_the_header_is_pedantic_c99_with_the_tapfit_calls(pkg, tmp_path):
    src = tmp_path / "tapfit_probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "tapfit_probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    inv = pkg.GDG_ERR_INVALID
    assert [int(v) for v in lines[0].split()] == [inv, 0, inv, inv, inv]             # no context: refused, nothing touched; no fits in force
    assert lines[1] == "0 0.5 3" and lines[2] == "4 128 16"


def test_every_layer_knows_the_calls_and_prototypes_equal_exports(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in exported and name in pkg.ABI_SYMBOLS and re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
    assert {n for n in exported if n.startswith("gdg_") and "tapfit" in n} == set(NEW)
    for name in ("batch_tapfit_enable", "batch_tapfits", "batch_tapfit", "block_tapfit", "block_tapfit_device"):
        assert callable(getattr(pkg.Context, name)), name
    assert callable(pkg.blend_taps_from_tapfit) and callable(pkg.tapfit_doubles)
    assert (pkg.TAPFIT_MAX_TERMS, pkg.TAPFIT_MAX_UNKNOWNS, pkg.TAPFIT_MAX_FITS) == (4, 128, 16)
    flat = " ".join(header.replace(" * ", " ").split())
    for phrase in ("Nothing outside [first, first + L) is ever read", "L < T: every entry is +0.0", "positions behind L - T count as +0.0",
                   "With T = 1 and different ports the record is bit for bit the gdg_block_gram_rows record of the list",
                   "bit for bit what gdg_block_gram_rows returns for the V shifted rows written out on the host",
                   "GDG_ERR_UNSUPPORTED while tap fits are in force", "never collect tap-fit records", "ill-conditioned", "ridge > 0 is the remedy"):
        assert phrase in flat, phrase
    for macro, value in (("GDG_TAPFIT_MAX_TERMS", 4), ("GDG_TAPFIT_MAX_UNKNOWNS", 128), ("GDG_TAPFIT_MAX_FITS", 16)):
        assert re.search(r"^#define %s %d$" % (macro, value), header, re.M)
    with open(os.path.join(CSRC, "tapfit_kernels.h")) as f:
        kernel = f.read()
    assert re.search(r"^#define TAPFIT_KC %d\b" % pkg.TAPFIT_CHUNK, kernel, re.M), "TAPFIT_CHUNK is the kernel's chunk"
    with open(os.path.join(os.path.dirname(os.path.dirname(pkg.LIB_PATH)), "go", "gdg", "gdg.go")) as f:
        go = f.read()
    for sig in (r"^func \(this \*Context\) BatchTapFitEnable\(fits \[\]TapFit\) error", r"^func \(this \*Context\) BatchTapFits\(\) int",
                r"^func \(this \*Context\) BatchTapFit\(\) \(\[\]\[\]float64, error\)", r"^func \(this \*Context\) BlockTapFitRows\(", r"^func \(this \*Context\) BlockTapFitRowsDevice\(",
                r"^func TapFitDoubles\(fits \[\]TapFit\) int", r"^func BlendTapsFromTapFit\(records \[\]\[\]float64, fits \[\]TapFit, ridge float64\)"):
        assert re.search(sig, go, re.M), sig
    for name in NEW:
        assert "C.%s(" % name in go, name
    from go_dsp_guitar_amd import host
    assert callable(host.Engine._set_tapfits) and callable(host.Engine.render_tap_fitted) and host.lib().gdgh_engine_set_batch_tapfits is not None
    assert host.lib().gdgh_engine_last_batch_tapfit is not None
    with open(os.path.join(os.path.dirname(os.path.dirname(pkg.LIB_PATH)), "host", "gdg_host.hpp")) as f:
        hpp = f.read()
    assert "Error SetBatchTapFits(const std::vector<TapFit> &fits);" in hpp
    assert "Error LastBatchTapFit(std::vector<double> &records, size_t *blocks, size_t *doublesPerBlock) const;" in hpp
    assert os.path.exists(os.path.join(ROOT, "profiles", "probes", "batch_tapfit.py"))


def design_table():
    """the resources table of DESIGN.md 4.12g: {row name: text}"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    part = text[text.index("### 4.12g"):]
    assert "| | block_tapfit_kernel |" in part
    return dict(re.findall(r"^\| ([^|]+?) \| ([^|]+?) \|$", part, re.M))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_tapfit_kernel_uses_no_scratch_the_lds_of_the_table_and_the_f64_matrix_instruction(tmp_path):
    """block_tapfit_kernel from the compiler's resource summary: no scratch; LDS of five staged rows of 64 + 128 doubles, 7680 bytes, the
    figure DESIGN.md 4.12g states; and its instruction stream holds v_mfma_f64_16x16x4_f64, one accumulator x 32 steps per chunk."""
    out = str(tmp_path / "gram.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only", "-x", "hip",
                    os.path.join(CSRC, "gram.hip"), "-o", out], check=True, timeout=900, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @(.*?)^; TotalNumVgprs: (\d+).*?^; ScratchSize: (\d+).*?^; LDSByteSize: (\d+)", text, re.S | re.M):
        if "block_tapfit_kernel" in m.group(1):
            found[m.group(1)] = (int(m.group(3)), int(m.group(4)), int(m.group(5)), m.group(2).count("v_mfma_f64_16x16x4"))
    assert len(found) == 1, sorted(found)
    rows = design_table()
    stated = int(re.match(r"([\d ]+) bytes", rows["LDS"]).group(1).replace(" ", ""))
    for name, (vgprs, scratch, lds, mfma) in found.items():
        assert scratch == 0 and lds == 5 * (64 + 128) * 8 == stated and vgprs <= 128, (name, vgprs, scratch, lds, stated)
        assert mfma >= 1 and 128 // 4 % mfma == 0, (name, mfma)
