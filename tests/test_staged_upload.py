"""The native staged upload (csrc/hip/stage_upload.hip, csrc/stage_core.h)
and the sliced read through it: a background thread stages the file chunk by
chunk into pinned memory and enqueues each chunk's copy; the reader waits for
a slice to be issued, then gates its kernels on the slice's events.

The staged route is forced (_FORCE_STAGED), so the same code runs whether or
not the platform registers file mappings. Source `map` copies from the
file's real mapping, `pread` runs with the mapping pointer forced to 0. The
chunk size is patched down so that slices of 2-8 KiB hold one, two, or three
chunks plus a remainder. The oracle of the full reads is the one of
test_stream_decode.py: the unstreamed device decode, itself anchored to the
host codec. The thread's own hand-off logic is covered on the CPU by
csrc/tests/stage_selftest.cpp under the sanitizers.
"""

import os

import numpy as np
import pytest

import test_stream_decode as D
from spark_tfrecord_amd.engine import stream_plan

pytestmark = pytest.mark.gpu

SOURCES = ["map", "pread"]
# (slice, chunk): one chunk; two chunks; three chunks plus a remainder
LAYOUTS = [(2048, 2048), (4096, 2048), (8192, 2500)]


def _stage(monkeypatch, source, chunk):
    """Force the staged route with `source` and `chunk`; returns the list the
    StagedUpload objects of the reads that follow are appended to."""
    from spark_tfrecord_amd import _native
    g = D._g()
    monkeypatch.setattr(g, "_FORCE_STAGED", True)
    monkeypatch.setattr(g, "_STAGE_CHUNK", chunk)
    monkeypatch.setattr(g, "_STAGE_SOURCE", "map")
    if source == "pread":
        D._register_nothing(monkeypatch)  # mapping pointer 0
    made = []
    real = _native.StagedUpload

    def spy(fd, map_ptr, *rest):
        assert (map_ptr != 0) == (source == "map")
        made.append(real(fd, map_ptr, *rest))
        return made[-1]
    monkeypatch.setattr(_native, "StagedUpload", spy)
    return made


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("span,chunk", LAYOUTS)
@pytest.mark.parametrize("which", ["flagship", "one-byte"])
def test_upload_lands_every_byte(tmp_path, which, span, chunk, source):
    import torch
    from spark_tfrecord_amd import _native
    g = D._g()
    img = bytes(D._flagship()[0]) if which == "flagship" else b"\x5a"
    n = len(img)
    path = str(tmp_path / "u.bin")
    with open(path, "wb") as f:
        f.write(img)
    plan = stream_plan.plan_slices(n, span)
    bounds = [p.b0 for p in plan] + [n]
    mapped = _native.file_mmap_pinned(path, n, False)[0] if source == "map" else 0
    assert (mapped != 0) == (source == "map")
    stage = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    data = torch.zeros(n, dtype=torch.uint8, device="cuda")
    streams = g._dma_streams()
    main = torch.cuda.current_stream()
    for st in streams:
        st.wait_stream(main)  # the zero fill above
    fd = os.open(path, os.O_RDONLY)
    try:
        up = _native.StagedUpload(fd, mapped, stage.data_ptr(), data.data_ptr(),
                                  bounds, streams[0].cuda_stream,
                                  streams[1].cuda_stream, chunk, True,
                                  data.device.index)
        assert up.nslices == len(plan)
        assert up.nchunks == sum(-(-(p.b1 - p.b0) // chunk) for p in plan)
        try:
            for s in range(len(plan)):
                evs = up.wait_issued(s)  # host wait first, then the stream's
                assert len(evs) == 2 and up.issued > s
                for ev in evs:
                    _native.gpu_stream_wait_event(main.cuda_stream, ev)
            up.wait_all()
            with pytest.raises(IndexError):
                up.wait_issued(len(plan))
        finally:
            up.close()
        assert up.closed and up.issued == len(plan)
    finally:
        os.close(fd)
    got = data.cpu().numpy()  # on the main stream, behind the event waits
    assert np.array_equal(got, np.frombuffer(img, np.uint8))
    for st in streams:
        st.synchronize()  # `stage` is freed on return


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("chunk", [2048, 1024, 600])
def test_reads_equal_host_codec(tmp_path, monkeypatch, source, chunk):
    g = D._g()
    made = _stage(monkeypatch, source, chunk)
    want = D._check(tmp_path, monkeypatch, D._flagship(), 2 << 10, True, True,
                    min_slices=21)
    assert want.num_rows == 300
    assert len(made) == 1 and made[0].closed
    assert made[0].issued == made[0].nslices == g.last_read["slices"]
    assert g.last_read["host_waits"] <= g.last_read["slices"] + 3
    # again: the staging buffer is reused, now with a file of another size
    D._check(tmp_path, monkeypatch, D._ragged(), 8 << 10, True, True,
             min_slices=4)
    assert len(made) == 2 and made[1].closed
    assert made[1].issued == made[1].nslices


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("stream", [True, False])
def test_unstreamed_paths_use_the_upload(tmp_path, monkeypatch, source, stream):
    # the false-positive header leaves the streamed loop at the first slice
    # (fallback); TFREC_STREAM_DECODE=0 never enters it (unstreamed). Both
    # wait for all slices of the same object, whose thread is joined after.
    g = D._g()
    made = _stage(monkeypatch, source, 1500)
    img, schema = D._false_positive_file(2)
    want = D._oracle(img, schema, "Example", True)
    D._assert_matches_host_codec(want, img, schema, "Example", True)
    path = str(tmp_path / "u.tfrecord")
    with open(path, "wb") as f:
        f.write(img)
    monkeypatch.setattr(g, "_STREAM_DECODE", stream)
    monkeypatch.setattr(g, "_READ_SLICE", 4 << 10)
    g.last_read.clear()
    D._assert_same(g.read_file_to_batch_pipelined(path, schema, "Example"), want)
    assert g.last_read["path"] == ("fallback" if stream else "unstreamed")
    assert g.last_read["slices"] == 3
    assert len(made) == 1 and made[0].closed and made[0].issued == 3


@pytest.mark.parametrize("source", SOURCES)
def test_file_truncated_after_planning(tmp_path, monkeypatch, source):
    # The file loses its second half after the slice plan was made: the
    # thread's pread hits the end of the file (pread), or its size check
    # refuses the chunk before the mapping is touched (map). Host errors
    # only; the device sees the copies of the slices staged before it.
    from spark_tfrecord_amd import _native
    g = D._g()
    img, schema, rt = D._flagship()
    path = str(tmp_path / "t.tfrecord")
    with open(path, "wb") as f:
        f.write(img)
    if source == "map" and _native.file_mmap_pinned(path, len(img), False)[1]:
        pytest.skip("truncating a file under a registered mapping blocks")
    made = _stage(monkeypatch, source, 1024)
    monkeypatch.setattr(g, "_READ_SLICE", 4 << 10)
    real_plan = stream_plan.plan_slices

    def plan_then_truncate(n, span):
        plan = real_plan(n, span)
        os.truncate(path, n // 2)
        return plan
    monkeypatch.setattr(stream_plan, "plan_slices", plan_then_truncate)
    with pytest.raises(RuntimeError, match="staged read failed at byte"):
        g.read_file_to_batch_pipelined(path, schema, rt)
    assert len(made) == 1 and made[0].closed
    assert made[0].issued < made[0].nslices
    with pytest.raises(RuntimeError, match="staged read failed"):
        made[0].wait_all()
    # a good file in the same process reads fine afterwards
    monkeypatch.setattr(stream_plan, "plan_slices", real_plan)
    D._check(tmp_path, monkeypatch, (img, schema, rt), 4 << 10, True, True,
             min_slices=10)
    assert len(made) == 2 and made[1].closed
