"""The extraction kernels write finished columns: elem_off, sub_off (with
their end sentinels) and presence come straight out of extract_fields, no
prefix sum or elementwise kernel follows. Everything is compared with the
host codec, which still builds the same columns from lengths and counts. No
arithmetic is involved, so every comparison is exact.
"""

import numpy as np
import pytest

import spark_tfrecord_amd as stf
from spark_tfrecord_amd.columnar import RecordBatch, column_from_values
from spark_tfrecord_amd.engine import cpu as cpu_engine

pytestmark = pytest.mark.gpu

PARTS = ("presence", "row_off", "values", "elem_off", "list_off", "sub_off")
CANARY = -0x5A5A5A5A5A5A5A5B


def _g():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _batch(schema, columns):
    n = len(next(iter(columns.values())))
    cols = [column_from_values(columns[f.name], f.dataType, True, f.name)
            for f in schema.fields]
    return RecordBatch(schema, cols, n)


def _S(*fields):
    return stf.StructType([stf.StructField(n, t, True) for n, t in fields])


def _case_absent_everywhere():
    schema = _S(("id", stf.LongType()), ("s", stf.StringType()))
    img = cpu_engine.encode_batch(_batch(schema, {
        "id": list(range(300)), "s": [f"v{i}" for i in range(300)]}),
        "Example")
    # decode with a bytes field and a bytes list no record carries
    schema = _S(("id", stf.LongType()), ("ghost", stf.StringType()),
                ("s", stf.StringType()),
                ("ghosts", stf.ArrayType(stf.BinaryType())))
    return img, schema, "Example"


def _case_absent_at_the_end():
    n = 120
    schema = _S(("id", stf.LongType()), ("s", stf.StringType()),
                ("blobs", stf.ArrayType(stf.BinaryType())))
    img = cpu_engine.encode_batch(_batch(schema, {
        "id": list(range(n)),
        "s": [f"name-{i}" * (1 + i % 3) if i < n - 3 else None
              for i in range(n)],
        "blobs": [[b"q" * (i % 7), b"r" * (i % 3)] if i < n - 3 else None
                  for i in range(n)],
    }), "Example")
    return img, schema, "Example"


def _case_zero_length_strings():
    n = 150
    schema = _S(("s", stf.StringType()),
                ("blobs", stf.ArrayType(stf.BinaryType())))
    img = cpu_engine.encode_batch(_batch(schema, {
        "s": ["" if i % 2 else "x" * (i % 5) for i in range(n)],
        "blobs": [[b""] * (i % 4) + [b"z" * (i % 3)] for i in range(n)],
    }), "Example")
    return img, schema, "Example"


def _case_sequence_with_empties():
    n = 120
    rng = np.random.default_rng(9)
    schema = _S(("ctx", stf.LongType()),
                ("rag", stf.ArrayType(stf.ArrayType(stf.FloatType()))),
                ("toks", stf.ArrayType(stf.ArrayType(stf.StringType()))),
                ("ids", stf.ArrayType(stf.ArrayType(stf.LongType()))))
    img = cpu_engine.encode_batch(_batch(schema, {
        "ctx": [int(v) for v in rng.integers(0, 10, n)],
        # empty lists (i % 3 == 0) and empty sub-lists (j % 2 == 0)
        "rag": [[[0.5 * k for k in range(j % 2 * (1 + j))]
                 for j in range(i % 3)] for i in range(n)],
        "toks": [[[f"t{i}-{k}" * (k % 2) for k in range(j % 3)]
                  for j in range(i % 4)] for i in range(n)],
        "ids": [[list(range(j)) for j in range(i % 5)] if i % 7 else []
                for i in range(n)],
    }), "SequenceExample")
    return img, schema, "SequenceExample"


def _case_wave_kernels():
    # 12 KB records select the one-record-per-wave kernels
    schema = _S(("s", stf.StringType()), ("id", stf.LongType()))
    img = cpu_engine.encode_batch(_batch(schema, {
        "s": ["x" * (12_000 + 11 * i) if i < 37 else None for i in range(40)],
        "id": list(range(40))}), "Example")
    return img, schema, "Example"


CASES = {
    "absent_everywhere": (_case_absent_everywhere, 2 << 10),
    "absent_at_the_end": (_case_absent_at_the_end, 2 << 10),
    "zero_length_strings": (_case_zero_length_strings, 2 << 10),
    "sequence_with_empties": (_case_sequence_with_empties, 4 << 10),
    "wave_kernels": (_case_wave_kernels, 4 << 10),
}


def _assert_equals_host(batch, img, schema, record_type):
    host = cpu_engine.decode_buffer(np.frombuffer(img, np.uint8), schema,
                                    record_type, True)
    dev = _g().batch_to_host(batch)
    assert dev.num_rows == host.num_rows
    assert len(dev.columns) == len(host.columns)
    for f, a, b in zip(schema.fields, dev.columns, host.columns):
        for part in PARTS:
            va, vb = getattr(a, part), getattr(b, part)
            assert (va is None) == (vb is None), (f.name, part)
            if vb is not None:
                va, vb = np.asarray(va), np.asarray(vb)
                assert va.dtype == vb.dtype, (f.name, part)
                assert np.array_equal(va, vb), (f.name, part)
    return host


@pytest.mark.parametrize("name", list(CASES))
def test_decode_device_columns_equal_host_codec(name):
    import torch
    g = _g()
    img, schema, rt = CASES[name][0]()
    data = torch.frombuffer(bytearray(img), dtype=torch.uint8).cuda()
    off, lens = g.scan_frames_device(data)
    batch = g.decode_device(data, off, lens, schema, rt, True)
    host = _assert_equals_host(batch, img, schema, rt)
    if name == "absent_everywhere":
        assert np.array_equal(np.asarray(host.columns[1].elem_off), [0])
        assert batch.columns[1].elem_off.cpu().tolist() == [0]
        assert batch.columns[3].elem_off.cpu().tolist() == [0]


@pytest.mark.parametrize("extract", [True, False])
@pytest.mark.parametrize("name", list(CASES))
def test_streamed_columns_equal_host_codec(tmp_path, monkeypatch, name, extract):
    from spark_tfrecord_amd import _native
    g = _g()
    make, read_slice = CASES[name]
    img, schema, rt = make()
    path = str(tmp_path / "f.tfrecord")
    with open(path, "wb") as f:
        f.write(img)
    assert _native.file_mmap_pinned(path, len(img), False)[1]
    monkeypatch.setattr(g, "_STREAM_DECODE", True)
    monkeypatch.setattr(g, "_STREAM_EXTRACT", extract)
    monkeypatch.setattr(g, "_READ_SLICE", read_slice)
    g.last_read.clear()
    batch = g.read_file_to_batch_pipelined(path, schema, rt, verify_crc=True)
    assert g.last_read["path"] == "streamed"
    assert g.last_read["slices"] >= 3
    _assert_equals_host(batch, img, schema, rt)


# ---------------------------------------------------------------------------
# Ranged native extraction on canary-filled buffers
# ---------------------------------------------------------------------------

def _scanned(img, schema, record_type):
    """Frames, FieldStat rows and the three prefix planes of `img`."""
    import torch
    from spark_tfrecord_amd import _native
    from spark_tfrecord_amd.columnar import wire_fields
    g = _g()
    data = torch.frombuffer(bytearray(img), dtype=torch.uint8).cuda()
    off, lens = g.scan_frames_device(data)
    R, F = off.numel(), len(wire_fields(schema))
    blob = g._schema_blob_device(schema, data.device)
    stats = torch.empty((R, F, 6), dtype=torch.int64, device="cuda")
    err = torch.zeros(2, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _native.gpu_scan_records(data.data_ptr(), off.data_ptr(), lens.data_ptr(),
                             R, g.FMT[record_type], blob.data_ptr(), F,
                             stats.data_ptr(), err.data_ptr(), 0, stream, 0)
    planes = [torch.zeros((F, R + 1), dtype=torch.int64, device="cuda")
              for _ in range(3)]
    ws = g._stat_scan_workspace(R, F, data.device)
    _native.gpu_stat_scans(ws.data_ptr(), ws.numel(), stats.data_ptr(), R, F,
                           *[t.data_ptr() for t in planes], stream)
    assert err.cpu().tolist()[0] == 0
    return data, stats, planes, R, F


SLACK = 8  # canary elements past every buffer's last live slot


def _buffers(schema, planes, R):
    """Canary-filled destination buffers, SLACK elements longer than the
    totals at row R need; returns (per-field dicts, metas)."""
    import torch
    from spark_tfrecord_amd.columnar import wire_fields
    from spark_tfrecord_amd.schema import (KIND_BYTES, KIND_FLOAT, KIND_INT64,
                                           is_sequence_field, wire_kind_of)
    tot = [p[:, R].cpu().tolist() for p in planes]
    bufs, metas = [], []

    def full(n, dtype):
        t = torch.empty(n, dtype=dtype, device="cuda")
        t.view(torch.uint8).fill_(0xA5)
        return t

    for i, f in enumerate(wire_fields(schema)):
        kind, seq = wire_kind_of(f.dataType), is_sequence_field(f.dataType)
        nv, nb, nl = tot[0][i], tot[1][i], tot[2][i]
        b = {"presence": full(R + SLACK, torch.uint8)}
        if kind == KIND_INT64:
            b["i64_vals"] = full(nv + SLACK, torch.int64)
        elif kind == KIND_FLOAT:
            b["f32_vals"] = full(nv + SLACK, torch.float32)
        else:
            assert kind == KIND_BYTES
            b["bytes_data"] = full(nb + SLACK, torch.uint8)
            b["elem_off"] = full(nv + 1 + SLACK, torch.int64)
        if seq:
            b["sub_off"] = full(nl + 1 + SLACK, torch.int64)
        bufs.append(b)
        metas.append({
            "kind": kind, "is_seq": 1 if seq else 0,
            **{k: t.data_ptr() for k, t in b.items()},
            "val_base": planes[0][i].data_ptr(),
            "byte_base": planes[1][i].data_ptr(),
            "list_base": planes[2][i].data_ptr() if seq else 0,
        })
    return bufs, metas


def _extract(data, stats, metas, r0, r1, F, avg_bytes=0):
    import torch
    from spark_tfrecord_amd import _native
    meta_dev = torch.empty(F * _native.gpu_devmeta_bytes(), dtype=torch.uint8,
                           device="cuda")
    err = torch.zeros(2, dtype=torch.int32, device="cuda")
    _native.gpu_extract_fields(data.data_ptr(), r1 - r0, F, stats.data_ptr(),
                               metas, meta_dev.data_ptr(), err.data_ptr(),
                               torch.cuda.current_stream().cuda_stream,
                               avg_bytes, r0=r0)
    torch.cuda.synchronize()
    assert err.cpu().tolist()[0] == 0


def _ranged_example():
    n = 64
    rng = np.random.default_rng(3)
    schema = _S(("id", stf.LongType()), ("s", stf.StringType()),
                ("arr", stf.ArrayType(stf.LongType())),
                ("farr", stf.ArrayType(stf.FloatType())),
                ("blobs", stf.ArrayType(stf.BinaryType())))
    img = cpu_engine.encode_batch(_batch(schema, {
        "id": [int(i) if i % 5 else None for i in range(n)],
        "s": [f"name-{i}" * (i % 4) if i % 7 else None for i in range(n)],
        "arr": [list(range(i % 5)) for i in range(n)],
        "farr": [list(rng.random(i % 8).astype(float)) for i in range(n)],
        "blobs": [[b"k" * int(k) for k in rng.integers(0, 40, i % 3)]
                  for i in range(n)],
    }), "Example")
    return img, schema, "Example"


def _ranged_sequence():
    n = 64
    schema = _S(("ctx", stf.LongType()),
                ("rag", stf.ArrayType(stf.ArrayType(stf.FloatType()))),
                ("toks", stf.ArrayType(stf.ArrayType(stf.StringType()))))
    img = cpu_engine.encode_batch(_batch(schema, {
        "ctx": list(range(n)),
        "rag": [[[0.25 * k for k in range((i + j) % 4)] for j in range(i % 3)]
                for i in range(n)],
        "toks": [[[f"t{i}-{k}" for k in range(j % 3)] for j in range(i % 4)]
                 for i in range(n)],
    }), "SequenceExample")
    return img, schema, "SequenceExample"


@pytest.mark.parametrize("avg_bytes", [0, 1 << 20], ids=["lane", "wave"])
@pytest.mark.parametrize("make", [_ranged_example, _ranged_sequence],
                         ids=["example", "sequence"])
def test_two_ranged_calls_equal_one(make, avg_bytes):
    import torch
    img, schema, rt = make()
    data, stats, planes, R, F = _scanned(img, schema, rt)
    assert R == 64
    r = 23
    one, metas_one = _buffers(schema, planes, R)
    _extract(data, stats, metas_one, 0, R, F, avg_bytes)
    two, metas_two = _buffers(schema, planes, R)
    _extract(data, stats, metas_two, 0, r, F, avg_bytes)
    # after the first range: sentinels at the totals of row r, canary beyond
    for i, b in enumerate(two):
        nv, nb, nl = (int(p[i, r]) for p in planes)
        assert bool((b["presence"][r:] == 0xA5).all())
        if "elem_off" in b:
            assert int(b["elem_off"][nv]) == nb
            assert bool((b["elem_off"][nv + 1:] == CANARY).all())
            assert bool((b["bytes_data"][nb:] == 0xA5).all())
        if "sub_off" in b:
            assert int(b["sub_off"][nl]) == nv
            assert bool((b["sub_off"][nl + 1:] == CANARY).all())
    _extract(data, stats, metas_two, r, R, F, avg_bytes)
    checked = 0
    for i, (a, b) in enumerate(zip(one, two)):
        nv, nb, nl = (int(p[i, R]) for p in planes)
        live = {"presence": R, "i64_vals": nv, "f32_vals": nv,
                "bytes_data": nb, "elem_off": nv + 1, "sub_off": nl + 1}
        for name in a:
            ta, tb = a[name].view(torch.uint8), b[name].view(torch.uint8)
            assert torch.equal(ta, tb), (i, name)
            # nothing past the live slots (the sentinels included) is written
            tail = a[name][live[name]:].view(torch.uint8)
            assert tail.numel() == SLACK * a[name].element_size()
            assert bool((tail == 0xA5).all()), (i, name)
            checked += 1
    assert checked >= 2 * F
    # and the single call is the host codec's columns
    host = cpu_engine.decode_buffer(np.frombuffer(img, np.uint8), schema, rt,
                                    True)
    for i, (a, c) in enumerate(zip(one, host.columns)):
        nv, nl = int(planes[0][i, R]), int(planes[2][i, R])
        assert np.array_equal(a["presence"][:R].cpu().numpy(),
                              np.asarray(c.presence))
        if c.elem_off is not None:
            assert np.array_equal(a["elem_off"][:nv + 1].cpu().numpy(),
                                  np.asarray(c.elem_off))
        if c.sub_off is not None:
            assert np.array_equal(a["sub_off"][:nl + 1].cpu().numpy(),
                                  np.asarray(c.sub_off))
