"""CPU-side checks of the streamed form of a shard (gdg_batch_stream_open_shard / gdg_batch_stream_step_shard /
gdg_batch_finish_master_slice): declared in include/gdg.h, exported by libgdg.so, listed in ABI_SYMBOLS, called by the Go binding,
and carried by the C++ twin (gdgh_engine_batch_stream_sharded_*).  What the calls compute: tests/test_gpu_batch_stream_shard.py."""
import ctypes
import os
import re

import pytest

import __graft_entry__ as entry

ROOT = entry.ROOT
NAMES = ["gdg_batch_stream_open_shard", "gdg_batch_stream_step_shard", "gdg_batch_finish_master_slice"]
TWIN = ["gdgh_engine_batch_stream_sharded_open", "gdgh_engine_batch_stream_sharded_need", "gdgh_engine_batch_stream_sharded_step",
        "gdgh_engine_batch_stream_sharded_close"]


@pytest.fixture(scope="module")
def pkg():
    p = entry.load_package()
    p.build()
    return p


def header():
    return open(os.path.join(ROOT, "include", "gdg.h")).read()


@pytest.mark.parametrize("name", NAMES)
def test_the_call_is_declared_exported_and_listed(pkg, name):
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*gdg_ctx\s*\*" % name, code), "%s is not declared in include/gdg.h" % name
    assert hasattr(ctypes.CDLL(pkg.LIB_PATH), name), "libgdg.so does not export %s" % name
    assert name in pkg.ABI_SYMBOLS
    assert getattr(pkg.lib(), name).argtypes, "%s has no ctypes prototype" % name


def test_the_prototypes_have_the_arguments_of_their_one_call_forms():
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    args = lambda name: [a.strip() for a in re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, code, flags=re.S).group(1).split(",")]
    strip = lambda a: re.sub(r"\s+", " ", a)
    # the finish of a slice takes what the finish of a job takes
    assert [strip(a) for a in args("gdg_batch_finish_master_slice")] == [strip(a) for a in args("gdg_batch_finish_master")]
    assert len(args("gdg_batch_stream_open_shard")) == len(args("gdg_batch_stream_open")) + 2
    assert len(args("gdg_batch_stream_step_shard")) == len(args("gdg_batch_stream_step")) + 1
    assert "gdg_batch_shard_out" in args("gdg_batch_stream_step_shard")[-1]


def test_the_header_describes_the_streamed_shard():
    text = header()
    assert "does not exist yet" not in text
    assert re.search(r"one\s+call\s+at\s+a\s+time", text, flags=re.I), "the header must say that a context runs one call at a time"


def test_the_python_binding_has_the_methods(pkg):
    for method in ("batch_stream_open_shard", "batch_stream_step_shard", "batch_finish_master_slice", "batch_stream_shard"):
        assert callable(getattr(pkg.Context, method, None)), method


def test_the_go_binding_calls_each_of_the_three():
    src = open(os.path.join(entry.PKG_DIR, "go", "gdg", "gdg.go")).read()
    for name in NAMES:
        assert re.search(r"\bC\.%s\(" % name, src), "gdg.go never calls %s" % name
    for func in ("BatchStreamOpenShard", "BatchStreamStepShard", "FinishMasterSlice"):
        assert re.search(r"^func \(this \*Context\) %s\(" % func, src, flags=re.M), func
    assert re.search(r"^func \(this \*Context\) BatchStreamStepShard\([^)]*\) \(\*ShardResult, error\)", src, flags=re.M)


def test_the_twin_exports_the_sharded_streamed_run(pkg):
    from go_dsp_guitar_amd import host
    host.build()
    lib = ctypes.CDLL(host.LIB_PATH)
    for name in TWIN:
        assert hasattr(lib, name), "libgdg_host.so does not export %s" % name
    assert callable(getattr(host.Engine, "batch_stream_sharded", None))
