"""Engine::BatchStreamShardedOpen / Need / Step / Close of the C++ twin (host/gdg_host.hpp): the streamed run of an engine of ANY shard
count -- every shard streams its channels (gdg_batch_stream_open_shard / _step_shard), the master is finished per slice
(gdg_batch_finish_master_slice) -- has the bytes of Engine::BatchRun on an identically built engine."""
import numpy as np
import pytest

from test_host_mirror_batch_stream import BLOCK, _engine, _files, host  # noqa: F401 (host: the module's fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]], ids=["one-shard", "two-shards", "three-shards"])
def test_engine_sharded_streamed_job_has_the_bytes_of_batch_run(host, oracle, devices):
    sr, nch = 48000, 4
    inputs = _files(oracle, sr)
    eng, sp = _engine(host, nch, sr, devices=devices)
    assert eng.shards() == len(devices)
    want = eng.batch_run(inputs, sr, "lpcm24", window=4, metronome_to_master=True)
    assert eng.last_error() == ""
    del sp
    eng.close()
    blocks = want[0].size // 3 // BLOCK
    assert blocks >= 8
    for slicing in ([3] * (blocks // 3) + [blocks % 3] * (blocks % 3 > 0), [1, 4, 2] + [blocks - 7]):
        assert sum(slicing) == blocks
        eng, sp = _engine(host, nch, sr, devices=devices)
        it = iter(slicing)
        parts = list(eng.batch_stream_sharded(inputs, sr, "lpcm24", lambda left: next(it), window=4, metronome_to_master=True))
        assert eng.last_error() == ""
        assert [p[0].size for p in parts] == [k * BLOCK * 3 for k in slicing]
        for r in range(nch + 3):
            np.testing.assert_array_equal(np.concatenate([p[r] for p in parts]), want[r], err_msg="output %d, slices %s, %d shards" % (r, slicing, len(devices)))
        del sp
        eng.close()


def test_engine_sharded_stream_refuses_what_is_not_open(host, oracle):
    sr, nch = 48000, 4
    eng, sp = _engine(host, nch, sr, devices=[0, 0])
    gen = eng.batch_stream_sharded(_files(oracle, sr), sr, "lpcm24", 2, window=4)
    first = next(gen)
    assert len(first) == nch + 3
    with pytest.raises(host.HostError, match="already open"):
        next(eng.batch_stream_sharded(_files(oracle, sr), sr, "lpcm24", 2, window=4))
    second = next(gen)                                              # the refused open left the job alone
    assert second[0].size == first[0].size
    gen.close()                                                     # closes the job on every shard
    assert len(list(eng.batch_stream_sharded(_files(oracle, sr), sr, "lpcm24", 5, window=4))) == 2      # ... and the engine takes the next one
    del sp
    eng.close()
