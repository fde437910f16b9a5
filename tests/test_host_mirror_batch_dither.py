"""Dither through the C++ twin (Engine::SetBatchDither, host.py's dither= argument): the engine gives every shard the job-wide index of its
first channel as port_base and keeps the master cursor over the slices, so a two-shard job writes the files of the one-shard job -- chain
outputs and metronome byte for byte (the master's sums are associated differently over two shards: it is held against the same engine's
one-call run instead) -- and the streamed sharded job writes the one-call job's seven files."""
import numpy as np
import pytest

import dither_ref as ref
from helpers import synth_signal
from test_host_mirror_batch_stream import BLOCK, _engine, host  # noqa: F401 (host: the module's fixture)

pytestmark = pytest.mark.gpu

SEED = 0x0123456789abcdef


def _inputs(sr, nch, blocks=3):
    enc = lambda x: np.ascontiguousarray(np.round(np.clip(x, -1, 1) * 32767.0).astype("<i2")).view(np.uint8)
    return [(enc(0.7 * synth_signal(c, blocks * BLOCK - 100 * c, sr)), "lpcm16", sr) for c in range(nch)]


def test_two_shards_with_dither_write_the_one_shard_files(host):
    sr, nch = 48000, 4
    inputs = _inputs(sr, nch)
    runs = {}
    kw = dict(window=2, metronome_to_master=True)
    for name, devices, fmt, dither in (("one", None, "lpcm16", SEED), ("rows", None, "ieee64", SEED), ("two", [0, 0], "lpcm16", SEED),
                                       ("two, streamed", [0, 0], "lpcm16", SEED), ("two, other seed", [0, 0], "lpcm16", SEED + 1),
                                       ("two, off", [0, 0], "lpcm16", None)):
        eng, sp = _engine(host, nch, sr, devices=devices)          # a fresh engine per job: the units start from rest
        assert eng.shards() == (1 if devices is None else 2)
        if name == "two, streamed":
            it = iter([1, 2])
            parts = list(eng.batch_stream_sharded(inputs, sr, fmt, lambda left: next(it), dither=dither, **kw))
            runs[name] = [np.concatenate([p[r] for p in parts]) for r in range(nch + 3)]
        else:
            runs[name] = [o.copy() for o in eng.batch_run(inputs, sr, fmt, dither=dither, **kw)]
        assert eng.last_error() == ""
        del sp
        eng.close()
    rows = [o.view(np.float64) for o in runs["rows"]]             # the float64 rows of the job: IEEE64 out is never dithered
    for r in list(range(nch)) + [nch + 2]:
        assert np.array_equal(runs["two"][r], runs["one"][r]), "output %d" % r
        assert not np.array_equal(runs["two"][r], runs["two, other seed"][r]), r
        assert not np.array_equal(runs["two"][r], runs["two, off"][r]), r
    for r in range(nch + 3):
        assert np.array_equal(runs["two, streamed"][r], runs["two"][r]), "streamed, output %d" % r
    # ... and they are the restatement of the rows: chain output c is port c whatever shard it ran on
    ports = list(range(nch)) + [ref.PORT_LEFT, ref.PORT_RIGHT, ref.PORT_METRONOME]
    for r in range(nch + 3):
        assert np.array_equal(runs["one"][r], ref.encode("lpcm16", rows[r], SEED, ports[r], 0)), "one shard against the restatement, output %d" % r


def test_a_resumed_sharded_job_goes_on_with_the_same_noise(host):
    """Slice 1 on one two-shard engine, a checkpoint, slices 2 and 3 on a fresh engine: all seven files are the uninterrupted job's.  The
    master's are the point -- the fresh engine's finishing context starts its cursor at the samples done, while its own job is open."""
    sr, nch = 48000, 4
    inputs = _inputs(sr, nch)
    kw = dict(window=2, metronome_to_master=True, dither=SEED)
    eng, sp = _engine(host, nch, sr, devices=[0, 0])
    want = [o.copy() for o in eng.batch_run(inputs, sr, "lpcm16", **kw)]
    del sp
    eng.close()
    eng, sp = _engine(host, nch, sr, devices=[0, 0])
    gen = eng.batch_stream_sharded(inputs, sr, "lpcm16", 1, **kw)
    head = [o.copy() for o in next(gen)]
    blob = eng.batch_stream_sharded_checkpoint()
    gen.close()                                                    # closes the job
    del sp
    eng.close()
    eng, sp = _engine(host, nch, sr, devices=[0, 0])
    tail = list(eng.batch_stream_sharded(inputs, sr, "lpcm16", 1, resume=blob, **kw))
    assert len(tail) == 2 and eng.last_error() == ""
    del sp
    eng.close()
    for r in range(nch + 3):
        got = np.concatenate([head[r]] + [p[r] for p in tail])
        assert np.array_equal(got, want[r]), "output %d: %d bytes differ" % (r, np.count_nonzero(got != want[r]))
