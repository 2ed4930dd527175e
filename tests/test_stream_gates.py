"""Device-side gates of the streamed read, called natively on R = 64 records:
the structure scan returns untouched when the broken-chain word is set, the
gated extraction writes nothing and raises the "not extracted" word unless
the chain holds, the scan was clean and every total fits its buffer. Plus
the bound on how often the streamed read blocks on the device.
"""

import numpy as np
import pytest

import spark_tfrecord_amd as stf
from spark_tfrecord_amd.columnar import RecordBatch, column_from_values
from spark_tfrecord_amd.engine import cpu as cpu_engine

pytestmark = pytest.mark.gpu

R = 64
WAVE = 1 << 20  # an avg_bytes that selects the one-record-per-wave kernels
KERNELS = pytest.mark.parametrize("avg_bytes", [0, WAVE], ids=["lane", "wave"])


def _g():
    from spark_tfrecord_amd.engine import gpu
    return gpu


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _file():
    """64 SequenceExamples: an int64, a float-list-list and a string-list-list
    field, so that every buffer kind and capacity is in play."""
    schema = stf.StructType([
        stf.StructField("ctx", stf.LongType(), True),
        stf.StructField("rag", stf.ArrayType(stf.ArrayType(stf.FloatType())), True),
        stf.StructField("toks", stf.ArrayType(stf.ArrayType(stf.StringType())), True),
    ])
    cols = {
        "ctx": list(range(R)),
        "rag": [[[0.25 * k for k in range((i + j) % 4)] for j in range(i % 3)]
                for i in range(R)],
        "toks": [[[f"t{i}-{k}" for k in range(j % 3)] for j in range(1 + i % 4)]
                 for i in range(R)],
    }
    batch = RecordBatch(schema, [
        column_from_values(cols[f.name], f.dataType, True, f.name)
        for f in schema.fields], R)
    return cpu_engine.encode_batch(batch, "SequenceExample"), schema


class _Scan:
    """The file on the device with its frames; scan() runs the structure
    scan into a given stats tensor."""

    def __init__(self):
        import torch
        g = _g()
        img, self.schema = _file()
        self.data = torch.frombuffer(bytearray(img), dtype=torch.uint8).cuda()
        self.off, self.lens = g.scan_frames_device(self.data)
        assert self.off.numel() == R
        self.F = 3
        self.blob = g._schema_blob_device(self.schema, self.data.device)

    def scan(self, stats, avg_bytes, gate=None, crc=None):
        import torch
        from spark_tfrecord_amd import _native
        err = torch.zeros(2, dtype=torch.int32, device="cuda")
        kw = {} if gate is None else {"gate": gate.data_ptr()}
        _native.gpu_scan_records(
            self.data.data_ptr(), self.off.data_ptr(), self.lens.data_ptr(), R,
            _g().FMT["SequenceExample"], self.blob.data_ptr(), self.F,
            stats.data_ptr(), err.data_ptr(),
            crc.data_ptr() if crc is not None else 0, _stream(), avg_bytes,
            **kw)
        torch.cuda.synchronize()
        return err.cpu().tolist()


@pytest.fixture(scope="module")
def scanned():
    import torch
    from spark_tfrecord_amd import _native
    g = _g()
    s = _Scan()
    s.stats = torch.empty((R, s.F, 6), dtype=torch.int64, device="cuda")
    assert s.scan(s.stats, 0) == [0, 0]
    s.planes = [torch.zeros((s.F, R + 1), dtype=torch.int64, device="cuda")
                for _ in range(3)]
    ws = g._stat_scan_workspace(R, s.F, s.data.device)
    _native.gpu_stat_scans(ws.data_ptr(), ws.numel(), s.stats.data_ptr(), R,
                           s.F, *[t.data_ptr() for t in s.planes], _stream())
    s.totals = [p[:, R].cpu().tolist() for p in s.planes]
    return s


@KERNELS
@pytest.mark.parametrize("crc", [False, True], ids=["nocrc", "crc"])
def test_scan_gate(scanned, avg_bytes, crc):
    import torch
    s = scanned

    def crc_word():
        return torch.full((1,), -1, dtype=torch.int64, device="cuda") \
            if crc else None

    canary = torch.full((R, s.F, 6), -7, dtype=torch.int64, device="cuda")
    gate = torch.ones(1, dtype=torch.int64, device="cuda")
    word = crc_word()
    assert s.scan(canary, avg_bytes, gate, word) == [0, 0]
    assert bool((canary == -7).all())  # broken chain: stats untouched
    if crc:
        assert int(word.item()) == -1
    gate.zero_()
    word = crc_word()
    assert s.scan(canary, avg_bytes, gate, word) == [0, 0]
    assert torch.equal(canary, s.stats)  # open gate == the ungated call
    if crc:
        assert int(word.item()) == -1


def _buffers(s):
    """Canary-filled, exactly sized destination buffers and their metas,
    capacities included."""
    import torch
    from spark_tfrecord_amd.schema import KIND_BYTES, KIND_FLOAT, KIND_INT64

    def full(n, dtype):
        t = torch.empty(max(n, 1), dtype=dtype, device="cuda")
        t.view(torch.uint8).fill_(0xA5)
        return t

    kinds = [(KIND_INT64, 0), (KIND_FLOAT, 1), (KIND_BYTES, 1)]
    bufs, metas = [], []
    for i, (kind, seq) in enumerate(kinds):
        nv, nb, nl = s.totals[0][i], s.totals[1][i], s.totals[2][i]
        b = {"presence": full(R, torch.uint8)}
        m = {"kind": kind, "is_seq": seq, "cap_vals": 0, "cap_bytes": 0,
             "cap_elem_off": 0, "cap_sub_off": 0}
        if kind == KIND_BYTES:
            b["bytes_data"] = full(nb, torch.uint8)
            b["elem_off"] = full(nv + 1, torch.int64)
            m.update(cap_bytes=nb, cap_elem_off=nv + 1)
        else:
            b["i64_vals" if kind == KIND_INT64 else "f32_vals"] = full(
                nv, torch.int64 if kind == KIND_INT64 else torch.float32)
            m.update(cap_vals=nv)
        if seq:
            b["sub_off"] = full(nl + 1, torch.int64)
            m.update(cap_sub_off=nl + 1)
        m.update({k: t.data_ptr() for k, t in b.items()})
        m.update(val_base=s.planes[0][i].data_ptr(),
                 byte_base=s.planes[1][i].data_ptr(),
                 list_base=s.planes[2][i].data_ptr() if seq else 0)
        bufs.append(b)
        metas.append(m)
    return bufs, metas


def _status():
    """(broken, crc, scan error pair, verdict) words of a clean read; the
    verdict starts at a value the gate never writes."""
    import torch
    st = torch.zeros(4, dtype=torch.int64, device="cuda")
    st[1] = -1
    st[3] = 99
    return st


def _extract(s, metas, avg_bytes, status=None):
    import torch
    from spark_tfrecord_amd import _native
    meta_dev = torch.empty(s.F * _native.gpu_devmeta_bytes(),
                           dtype=torch.uint8, device="cuda")
    xerr = torch.zeros(2, dtype=torch.int32, device="cuda")
    kw = {}
    if status is not None:
        p = status.data_ptr()
        kw = dict(gate_broken=p, gate_crc=p + 8, gate_err=p + 16,
                  gate_out=p + 24)
    _native.gpu_extract_fields(s.data.data_ptr(), R, s.F, s.stats.data_ptr(),
                               metas, meta_dev.data_ptr(), xerr.data_ptr(),
                               _stream(), avg_bytes, **kw)
    torch.cuda.synchronize()
    assert xerr.cpu().tolist() == [0, 0]


def _untouched(bufs):
    import torch
    return all(bool((t.view(torch.uint8) == 0xA5).all())
               for b in bufs for t in b.values())


@KERNELS
def test_clean_gate_equals_ungated_call(scanned, avg_bytes):
    import torch
    s = scanned
    plain, metas = _buffers(s)
    _extract(s, metas, avg_bytes)
    assert not _untouched(plain)
    gated, metas = _buffers(s)
    st = _status()
    _extract(s, metas, avg_bytes, st)
    assert st.cpu().tolist() == [0, -1, 0, 0]  # extracted
    for a, b in zip(plain, gated):
        for name in a:
            assert torch.equal(a[name].view(torch.uint8),
                               b[name].view(torch.uint8)), name


# (field, capacity) pairs: each is the one capacity that field's totals need
SHORT = [(0, "cap_vals"), (1, "cap_vals"), (1, "cap_sub_off"),
         (2, "cap_bytes"), (2, "cap_elem_off"), (2, "cap_sub_off")]


@KERNELS
@pytest.mark.parametrize("field,cap", SHORT,
                         ids=[f"f{f}-{c}" for f, c in SHORT])
def test_capacity_one_short_extracts_nothing(scanned, avg_bytes, field, cap):
    s = scanned
    bufs, metas = _buffers(s)
    assert metas[field][cap] >= 1
    metas[field][cap] -= 1
    st = _status()
    _extract(s, metas, avg_bytes, st)
    assert st.cpu().tolist() == [0, -1, 0, 1]  # not extracted
    assert _untouched(bufs)


@KERNELS
@pytest.mark.parametrize("word,value", [(0, 1), (1, 5), (2, 3)],
                         ids=["broken", "crc", "scan_error"])
def test_unclean_status_extracts_nothing(scanned, avg_bytes, word, value):
    s = scanned
    bufs, metas = _buffers(s)
    st = _status()
    st[word] = value
    want = st.cpu().tolist()
    _extract(s, metas, avg_bytes, st)
    want[3] = 1  # not extracted; the other words are only read
    assert st.cpu().tolist() == want
    assert _untouched(bufs)


@pytest.mark.parametrize("extract", [True, False])
def test_one_wait_per_slice(tmp_path, monkeypatch, extract):
    from bench import make_batch
    from spark_tfrecord_amd import _native
    g = _g()
    b = make_batch(300, seed=5)
    img = cpu_engine.encode_batch(b, "Example")
    path = str(tmp_path / "f.tfrecord")
    with open(path, "wb") as f:
        f.write(img)
    assert _native.file_mmap_pinned(path, len(img), False)[1]
    monkeypatch.setattr(g, "_STREAM_DECODE", True)
    monkeypatch.setattr(g, "_STREAM_EXTRACT", extract)
    monkeypatch.setattr(g, "_READ_SLICE", 2 << 10)
    g.last_read.clear()
    batch = g.read_file_to_batch_pipelined(path, b.schema, "Example",
                                           verify_crc=True)
    assert batch.num_rows == 300
    lr = g.last_read
    assert lr["path"] == "streamed"
    assert lr["slices"] >= 21
    # one wait per slice, the first extraction's sizing, the final snapshot
    # and the rare exact-regrow path
    assert lr["host_waits"] <= lr["slices"] + 3, lr
    host = cpu_engine.decode_buffer(np.frombuffer(img, np.uint8), b.schema,
                                    "Example", True)
    dev = g.batch_to_host(batch)
    for a, c in zip(dev.columns, host.columns):
        assert np.array_equal(np.asarray(a.values), np.asarray(c.values))
