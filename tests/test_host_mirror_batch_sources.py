"""Shared sources through the C++ twin (Engine::SetBatchSources, host.py's batch_set_sources): the map is given in JOB channel numbers and
split per shard; a two-shard engine's mapped job writes the bytes of the job with duplicated entries, and a reader whose root lives on
another shard is refused with a message."""
import pytest

from test_host_mirror_batch_stream import _engine, _files, host  # noqa: F401 (host: the module's fixture)

pytestmark = pytest.mark.gpu


def test_two_shards_mapped_job_equals_the_duplicated_job(host, oracle):
    sr, nch = 48000, 4
    files = _files(oracle, sr)                                     # 48 kHz, 44.1 kHz, empty, 96 kHz
    a, b = files[0], files[1]
    results = []
    for inputs, source in (([a, a, b, b], None), ([a, None, b, None], [0, 0, 2, 2])):
        eng, sp = _engine(host, nch, sr, devices=[0, 0])
        assert eng.shards() == 2 and eng.shard_range(1) == (2, 2)
        if source is not None:
            with pytest.raises(host.HostError, match="shard"):
                eng.batch_set_sources([0, 0, 0, 2])                # channel 2 (shard 1) reads channel 0 (shard 0)
            with pytest.raises(host.HostError, match="4 channels"):
                eng.batch_set_sources([0, 0])
            eng.batch_set_sources(source)
        results.append([o.tobytes() for o in eng.batch_run(inputs, sr, "lpcm24", window=4, metronome_to_master=True)])
        assert eng.last_error() == ""
        del sp
        eng.close()
    assert len(results[0]) == nch + 3 and results[1] == results[0]
    assert any(results[0][1]) and results[0][0] != results[0][1], "the readers' channels carry their own chains' outputs"
