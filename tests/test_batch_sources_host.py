"""The CPU side of shared sources (gdg_batch_set_sources): the pure host code behind the map -- validation, readers -> roots, per root the
rows it feeds (csrc/batch_sources.h) -- driven by a stand-alone program under AddressSanitizer and UBSan, and the entry point in every
layer: exported, declared as plain C, known to the Python layer, the Go binding and the C++ twin.  What the kernels write is
tests/test_gpu_batch_sources.py's business."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT

C_PROBE = r"""
#include <stdio.h>
#include "gdg.h"
int main(void) {
    const int map[2] = { 0, 0 };
    printf("%d %d\n", gdg_batch_set_sources(NULL, map, 2), gdg_batch_set_sources(NULL, NULL, 0));
    return 0;
}
"""


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


@pytest.fixture(scope="module")
def sources_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sources") / "sources_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "go-dsp-guitar_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "sources_check.cpp"), "-o", exe], check=True, timeout=300)
    return exe


@pytest.mark.parametrize("seed", [1, 2])
def test_map_bookkeeping_on_the_host(sources_check, seed):
    """hand-written maps (the refusals name the first offending channel) and 1500 random ones of up to 600 channels"""
    r = subprocess.run([sources_check, str(seed), "1500"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr


def test_the_call_links_from_c_and_refuses_no_context(pkg, tmp_path):
    src = tmp_path / "sources_probe.c"
    src.write_text(C_PROBE)
    exe = tmp_path / "sources_probe"
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
           "-L", lib_dir, "-lgdg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert [int(v) for v in r.stdout.split()] == [pkg.GDG_ERR_INVALID] * 2


def test_every_layer_knows_the_call_and_the_header_states_its_limits(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "gdg_batch_set_sources" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "gdg_batch_set_sources" in pkg.ABI_SYMBOLS and pkg.lib().gdg_batch_set_sources.argtypes is not None
    assert callable(pkg.Context.batch_set_sources)
    assert {"stat_batch_upload_bytes", "stat_batch_resampled_samples"} <= set(pkg.option_names())
    with open(os.path.join(ROOT, "include", "gdg.h")) as f:
        header = f.read()
    assert re.search(r"^int gdg_batch_set_sources\(gdg_ctx \*ctx, const int \*source, int n\);", header, re.M)
    for phrase in ("cannot be checkpointed yet", "computes the job's length over", "count[c] == 0 for a reader"):
        assert phrase in " ".join(header.replace(" * ", " ").split()), phrase
    base = os.path.dirname(os.path.dirname(pkg.LIB_PATH))
    with open(os.path.join(base, "go", "gdg", "gdg.go")) as f:
        go = f.read()
    assert re.search(r"^func \(this \*Context\) BatchSetSources\(source \[\]int\) error", go, re.M) and "C.gdg_batch_set_sources(" in go
    with open(os.path.join(base, "host", "gdg_host.hpp")) as f:
        hpp = f.read()
    with open(os.path.join(base, "host", "gdg_host.cpp")) as f:
        cpp = f.read()
    assert "Error SetBatchSources(const std::vector<int> &source)" in hpp
    assert re.search(r"^Error Engine::SetBatchSources\(", cpp, re.M) and "gdg_batch_set_sources(" in cpp
    from go_dsp_guitar_amd import host
    assert callable(host.Engine.batch_set_sources)
