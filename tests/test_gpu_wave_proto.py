"""Differential tests for the one-record-per-wave proto kernels.

Above 8 KiB of average record size every launcher in csrc/hip/kernels.hip
switches to a *_wave_kernel whose protobuf walk is written by hand and shares
nothing with csrc/codec_core.h. Here hand-built wire images are decoded and
encoded three ways: by the wave kernels, by the per-lane kernels and by the
host codec. The same "interesting" records are framed twice: alone (per-lane
kernels) and followed by one big padding record that lifts the average record
size over the threshold (wave kernels). No arithmetic is involved, so every
comparison is exact.

The tests without the gpu mark check the oracle itself: the host codec must
decode every hand-built image to the Python values written next to it, and
must refuse every malformed one.
"""

import functools
import itertools
import struct

import numpy as np
import pytest

import spark_tfrecord_amd as stf
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.columnar import (RecordBatch, WireColumn,
                                         column_from_values)
from spark_tfrecord_amd.engine import cpu as cpu_engine
from spark_tfrecord_amd.infer import byte_array_schema

gpu = pytest.mark.gpu

WAVE_BYTES = 8 << 10  # kWaveRecordBytes in csrc/hip/kernels.hip
PARTS = ("presence", "row_off", "values", "elem_off", "list_off", "sub_off")
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
PAD_KNOWN, PAD_UNKNOWN = "pad", "pad_not_in_schema"


def _g():
    from spark_tfrecord_amd.engine import gpu as g
    return g


# ---------------------------------------------------------------------------
# Wire builder
# ---------------------------------------------------------------------------

def varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def ld(fieldno, body):
    """A length-delimited field."""
    return varint((fieldno << 3) | 2) + varint(len(body)) + body


def frame(payload):
    header = struct.pack("<Q", len(payload))
    return (header + struct.pack("<I", _native.masked_crc32c(header)) + payload
            + struct.pack("<I", _native.masked_crc32c(payload)))


def packed(vals):
    return ld(1, b"".join(varint(v) for v in vals))


def unpacked(vals):
    return b"".join(b"\x08" + varint(v) for v in vals)


def packed_f(vals):
    return ld(1, struct.pack(f"<{len(vals)}f", *vals))


def unpacked_f(vals):
    return b"".join(b"\x0d" + struct.pack("<f", v) for v in vals)


def bytes_list(elems):
    return b"".join(ld(1, e) for e in elems)


BYTES, FLOAT, INT64 = 1, 2, 3  # Feature oneof field numbers


def feature(kind, list_body):
    return ld(kind, list_body)


def entry(name, value_body):
    return ld(1, ld(1, name.encode()) + ld(2, value_body))


def example(*entries):
    return ld(1, b"".join(entries))


def feature_list(*feature_bodies):
    return b"".join(ld(1, fb) for fb in feature_bodies)


def sequence_example(context_entries, list_entries):
    ctx = ld(1, b"".join(context_entries)) if context_entries else b""
    return ctx + ld(2, b"".join(list_entries))


# -- integer runs of an exact encoded length --------------------------------

def _s64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _of_width(k, top):
    """The largest (top) or smallest value whose varint takes k bytes."""
    if top:
        return -1 if k == 10 else _s64((1 << (7 * k)) - 1)
    return _s64(1 << (7 * (k - 1)))


ONES = [(37 * i + 1) % 128 for i in range(128)]
TENS = [-(i + 1) for i in range(50)] + [INT64_MIN]
WIDTHS = [_of_width(k, top) for k in range(1, 11) for top in (True, False)]
EXTREMES = [0, -1, INT64_MIN, INT64_MAX]
SOURCES = {"ones": ONES, "tens": TENS, "widths": WIDTHS, "extremes": EXTREMES}
RUN_BYTES = (1, 10, 63, 64, 65, 127, 128, 129, 640, 641, 1279)


def run_of(n, source):
    """Values cycled from `source` whose packed encoding is exactly n bytes;
    the last one is narrowed to the bytes that are left."""
    vals, left = [], n
    for v in itertools.cycle(source):
        if left == 0:
            break
        w = len(varint(v))
        if w > left:
            v, w = _of_width(left, False), left
        vals.append(v)
        left -= w
    assert sum(len(varint(v)) for v in vals) == n
    return vals


# one 1-byte value, then 10-byte values: 761 bytes, 12 per lane, and every
# lane boundary (a multiple of 12) falls inside a varint (starts are 0 and
# 1 + 10 j, all odd but 0)
INSIDE_RUN = [7] + [-(i + 2) for i in range(76)]
# 10-byte values, 640 bytes, 10 per lane: every boundary is a varint start
ALIGNED_RUN = run_of(640, TENS)


# ---------------------------------------------------------------------------
# The interesting records: (name, payload, {field: Python value})
# ---------------------------------------------------------------------------

def _S(*fields):
    return stf.StructType([stf.StructField(n, t, True) for n, t in fields])


L, F32, B = stf.LongType(), stf.FloatType(), stf.BinaryType()
A = stf.ArrayType

EXAMPLE_SCHEMA = _S(("ints", A(L)), ("flts", A(F32)), ("blobs", A(B)),
                    (PAD_KNOWN, B))
SEQUENCE_SCHEMA = _S(("ctx", A(L)), ("sids", A(A(L))), ("sflts", A(A(F32))),
                     ("sblobs", A(A(B))), (PAD_KNOWN, B))


def _ints(vals):
    return entry("ints", feature(INT64, packed(vals)))


def _packed_cases():
    cases = []
    for src, n in itertools.product(SOURCES, RUN_BYTES):
        vals = run_of(n, SOURCES[src])
        cases.append((f"{src}-{n}", example(_ints(vals)), {"ints": vals}))
    cases.append(("boundaries-inside-varints", example(_ints(INSIDE_RUN)),
                  {"ints": INSIDE_RUN}))
    cases.append(("boundaries-on-varint-starts", example(_ints(ALIGNED_RUN)),
                  {"ints": ALIGNED_RUN}))
    tail = run_of(117, ONES) + [INT64_MIN]
    cases.append(("ends-in-ten-bytes", example(_ints(tail)), {"ints": tail}))
    cases.append(("empty-packed-field",
                  example(entry("ints", feature(INT64, b"\x0a\x00"))),
                  {"ints": []}))
    return cases


def _quarter(n, k=1):
    return [0.25 * k * (i - n // 2) for i in range(n)]


def _encoding_cases():
    rng = np.random.default_rng(17)
    c = []
    v = [1, -1, 300, INT64_MIN, 0]
    c.append(("unpacked-int64",
              example(entry("ints", feature(INT64, unpacked(v)))),
              {"ints": v}))
    c.append(("unpacked-float",
              example(entry("flts", feature(FLOAT, unpacked_f([0.5, -2.0])))),
              {"flts": [0.5, -2.0]}))
    c.append(("mixed-pieces", example(
        entry("ints", feature(INT64, packed([1, 2]) + unpacked([3])
                              + packed([-4, 1 << 40]) + unpacked([-5, 6]))),
        entry("flts", feature(FLOAT, packed_f([1.0]) + unpacked_f([2.0])
                              + packed_f([3.0, 4.0])))),
        {"ints": [1, 2, 3, -4, 1 << 40, -5, 6],
         "flts": [1.0, 2.0, 3.0, 4.0]}))
    r65, r10, r129 = (run_of(65, WIDTHS), run_of(10, TENS),
                      run_of(129, EXTREMES))
    c.append(("several-packed-chunks", example(
        entry("ints", feature(INT64, packed(r65) + packed(r10) + packed([])
                              + packed(r129)))),
        {"ints": r65 + r10 + r129}))
    # a packed float chunk of 4 k + 2 bytes: the host codec keeps the k whole
    # floats and drops the rest
    c.append(("ragged-packed-float", example(
        entry("flts", feature(FLOAT, ld(1, struct.pack("<2f", 1.5, -3.0)
                                        + b"\x01\x02") + packed_f([9.0])))),
        {"flts": [1.5, -3.0, 9.0]}))
    # varints no writer produces but every parser takes: zero-padded ones,
    # and a tenth byte with more than its lowest bit set (the rest is lost)
    odd = (b"\x80\x00" + b"\x81\x80\x00" + b"\xff" * 9 + b"\x7f"
           + b"\x80" * 9 + b"\x00" + b"\x85\x80\x80\x00")
    c.append(("non-canonical-varints", example(
        entry("ints", feature(INT64, ld(1, odd * 8) + ld(1, odd)))),
        {"ints": [0, 1, -1, 0, 5] * 9}))
    big = _quarter(131)
    c.append(("long-float-run", example(
        entry("blobs", feature(BYTES, bytes_list([b"abc"]))),
        entry("flts", feature(FLOAT, packed_f(big)))),
        {"blobs": [b"abc"], "flts": big}))
    # unknown fields at every level: varint, fixed64, length-delimited, fixed32
    junk = (b"\x10\x96\x01" + b"\x21" + b"\x11" * 8 + ld(3, b"skipme")
            + b"\x2d" + b"\x22" * 4)
    iv = run_of(70, WIDTHS)
    c.append(("unknown-fields", ld(2, b"top") + example(
        ld(2, b"in-features"),
        ld(1, ld(1, b"ints") + b"\x18\x07"
           + ld(2, ld(4, b"in-feature") + feature(
               INT64, junk + packed(iv[:3]) + junk + packed(iv[3:]))
               + b"\x48\x01")),
        ld(1, ld(1, b"blobs") + ld(2, feature(
            BYTES, junk + bytes_list([b"one"]) + junk + bytes_list([b""])))),
        ld(1, ld(1, b"flts") + ld(2, feature(
            FLOAT, packed_f([2.5]) + junk + unpacked_f([3.5]))))) + b"\x3d"
        + b"\x33" * 4,
        {"ints": iv, "blobs": [b"one", b""], "flts": [2.5, 3.5]}))
    c.append(("value-before-key", example(
        ld(1, ld(2, feature(INT64, packed([11, -12]))) + ld(1, b"ints")),
        ld(1, ld(2, feature(BYTES, bytes_list([b"vk"]))) + ld(1, b"blobs"))),
        {"ints": [11, -12], "blobs": [b"vk"]}))
    first, last = run_of(129, TENS), [5]
    c.append(("duplicate-key-shrinks", example(_ints(first), _ints(last)),
              {"ints": last}))
    c.append(("duplicate-key-grows", example(_ints(last), _ints(first)),
              {"ints": first}))
    c.append(("duplicate-key-to-empty", example(
        entry("blobs", feature(BYTES, bytes_list([b"gone"] * 3))),
        entry("blobs", b"")), {"blobs": []}))
    c.append(("feature-without-list", example(
        entry("ints", b""), entry("flts", b"\x48\x01"),
        entry("blobs", feature(BYTES, b""))),
        {"ints": [], "flts": [], "blobs": []}))
    c.append(("no-features", example(), {}))
    c.append(("empty-payload", b"", {}))
    blob = rng.bytes(300)
    c.append(("all-three", example(
        entry("blobs", feature(BYTES, bytes_list([blob, b"", blob[:9]]))),
        _ints([INT64_MAX, INT64_MIN]),
        entry("flts", feature(FLOAT, packed_f([-0.0, 1e30])))),
        {"blobs": [blob, b"", blob[:9]], "ints": [INT64_MAX, INT64_MIN],
         "flts": [-0.0, 1e30]}))
    return c


ELEM_BYTES = (0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513)


def _bytes_cases():
    """Eight records, each with all eleven element lengths, rotated, behind
    a leading element of k bytes: source and destination offsets of the long
    elements then take every residue mod 8 (checked by a test below)."""
    rng = np.random.default_rng(23)
    cases = []
    for k in range(8):
        lens = [k] + [ELEM_BYTES[(i + k) % 11] for i in range(11)]
        elems = [rng.bytes(n) for n in lens]
        cases.append((f"rotation-{k}", example(
            entry("blobs", feature(BYTES, bytes_list(elems)))),
            {"blobs": elems}))
    return cases


def _sequence_cases():
    rng = np.random.default_rng(29)
    c = []
    c.append(("nothing", sequence_example([], []), {}))
    c.append(("context-only", ld(1, entry("ctx", feature(INT64, packed([4])))),
              {"ctx": [4]}))
    c.append(("empty-feature-lists", sequence_example([], [
        entry("sids", b""), entry("sblobs", b""), entry("sflts", b"")]),
        {"sids": [], "sblobs": [], "sflts": []}))
    c.append(("empty-sub-lists", sequence_example([], [
        entry("sids", feature_list(feature(INT64, b""), b"",
                                   feature(INT64, packed([])))),
        entry("sblobs", feature_list(b"", feature(BYTES, b""))),
        entry("sflts", feature_list(feature(FLOAT, ld(1, b""))))]),
        {"sids": [[], [], []], "sblobs": [[], []], "sflts": [[]]}))
    subs = [run_of(63, WIDTHS), [], run_of(129, EXTREMES), [5, -5],
            run_of(641, WIDTHS), [INT64_MIN]]
    c.append(("int64-sub-lists", sequence_example(
        [entry("ctx", feature(INT64, packed(run_of(65, TENS))))],
        [entry("sids", feature_list(
            feature(INT64, packed(subs[0])), feature(INT64, b""),
            feature(INT64, packed(subs[2])), feature(INT64, unpacked(subs[3])),
            feature(INT64, packed(subs[4][:40]) + packed(subs[4][40:])),
            feature(INT64, packed(subs[5]))))]),
        {"ctx": run_of(65, TENS), "sids": subs}))
    blobs = [[b"", rng.bytes(65)], [], [rng.bytes(513), rng.bytes(7)],
             [rng.bytes(64)]]
    c.append(("bytes-sub-lists", sequence_example([], [
        entry("sblobs", feature_list(
            *[feature(BYTES, bytes_list(s)) for s in blobs]))]),
        {"sblobs": blobs}))
    flts = [_quarter(130), [], [1.5], _quarter(3, 5)]
    c.append(("float-sub-lists", sequence_example([], [
        entry("sflts", feature_list(
            feature(FLOAT, packed_f(flts[0])), feature(FLOAT, b""),
            feature(FLOAT, unpacked_f(flts[2])),
            feature(FLOAT, packed_f(flts[3]))))]),
        {"sflts": flts}))
    c.append(("unknown-fields-and-order", ld(3, b"top") + sequence_example(
        [ld(2, b"x"), entry("ctx", feature(INT64, packed([9])))],
        [b"\x19" + b"\x44" * 8,
         ld(1, ld(2, b"\x10\x05" + feature_list(
             feature(INT64, packed([1, 2])), feature(INT64, packed([-3])))
             + b"\x10\x06") + ld(1, b"sids")),
         entry("sblobs", feature_list(feature(BYTES, bytes_list([b"old"])))),
         entry("sblobs", feature_list(feature(BYTES, bytes_list([b"n"])),
                                      feature(BYTES, bytes_list([b"ew"]))))]),
        {"ctx": [9], "sids": [[1, 2], [-3]], "sblobs": [[b"n"], [b"ew"]]}))
    return c


PAYLOAD_BYTES = (0, 2, 63, 64, 65, 4095, 4096, 4097, 4160)


def _example_of(nbytes):
    """(payload, expectation) of an Example exactly nbytes long."""
    if nbytes == 0:
        return b"", {}
    if nbytes == 2:
        return example(), {}
    for extra in (b"", b"\x38\x01"):
        for n in range(max(0, nbytes - 40), nbytes):
            blob = bytes((7 * i + n) % 251 for i in range(n))
            p = example(entry("blobs", feature(BYTES, bytes_list([blob])))) + extra
            if len(p) == nbytes:
                return p, {"blobs": [blob]}
    raise AssertionError(nbytes)


def _size_cases():
    return [(f"payload-{n}",) + _example_of(n) for n in PAYLOAD_BYTES]


GROUPS = {
    "packed": ("Example", EXAMPLE_SCHEMA, _packed_cases),
    "encodings": ("Example", EXAMPLE_SCHEMA, _encoding_cases),
    "bytes": ("Example", EXAMPLE_SCHEMA, _bytes_cases),
    "sequence": ("SequenceExample", SEQUENCE_SCHEMA, _sequence_cases),
    "sizes": ("Example", EXAMPLE_SCHEMA, _size_cases),
}

# how an image is laid out: the records alone (per-lane kernels), or with the
# padding record behind them, its feature known or unknown to the schema, or
# in front of them (the streamed read settles the kernel set on the first
# records it sees)
LAYOUTS = ("lane", "wave-known", "wave-unknown", "wave-front")
WAVE_LAYOUTS = LAYOUTS[1:]


def _pad_payload(record_type, name, nbytes):
    body = bytes(i % 253 for i in range(nbytes))
    e = entry(name, feature(BYTES, bytes_list([body])))
    if record_type == "Example":
        return example(e), body
    return sequence_example([e], []), body


def _pad_bytes(payloads):
    """Padding that lifts len(img) // R - 16 over the threshold, with room."""
    R = len(payloads) + 1
    return R * (WAVE_BYTES + 96) - sum(len(p) + 16 for p in payloads)


def is_wave(img, R):
    """The launchers' rule (engine/gpu.py: avg_bytes; kernels.hip:
    kWaveRecordBytes)."""
    return len(img) // R - 16 > WAVE_BYTES


@functools.lru_cache(maxsize=None)
def image(group, layout):
    """(image, schema, record type, expected rows, index of the first
    interesting record)."""
    record_type, schema, make = GROUPS[group]
    cases = make()
    payloads = [p for _, p, _ in cases]
    rows = [dict(e) for _, _, e in cases]
    first = 0
    if layout != "lane":
        name = PAD_UNKNOWN if layout == "wave-unknown" else PAD_KNOWN
        pad, body = _pad_payload(record_type, name, _pad_bytes(payloads))
        pad_row = {PAD_KNOWN: [body]} if name == PAD_KNOWN else {}
        if layout == "wave-front":
            payloads, rows, first = [pad] + payloads, [pad_row] + rows, 1
        else:
            payloads, rows = payloads + [pad], rows + [pad_row]
    img = b"".join(frame(p) for p in payloads)
    assert is_wave(img, len(payloads)) == (layout != "lane")
    return img, schema, record_type, rows, first


# ---------------------------------------------------------------------------
# Column helpers
# ---------------------------------------------------------------------------

def rows_of(col):
    """A wire column as one Python value per row, from its offsets alone."""
    pres, ro = np.asarray(col.presence), np.asarray(col.row_off)
    vals = np.asarray(col.values)
    if col.kind == BYTES:
        eo = np.asarray(col.elem_off)
        assert len(eo) == ro[-1] + 1 and eo[-1] == len(vals)

        def elem(i):
            return vals[eo[i]:eo[i + 1]].tobytes()
    else:
        assert len(vals) == ro[-1]

        def elem(i):
            return vals[i].item()
    out = []
    for r in range(len(pres)):
        if not pres[r]:
            assert ro[r] == ro[r + 1]
            out.append(None)
        elif col.is_seq:
            lo, so = np.asarray(col.list_off), np.asarray(col.sub_off)
            assert so[lo[r]] == ro[r] and so[lo[r + 1]] == ro[r + 1]
            out.append([[elem(i) for i in range(so[j], so[j + 1])]
                        for j in range(lo[r], lo[r + 1])])
        else:
            out.append([elem(i) for i in range(ro[r], ro[r + 1])])
    return out


def _f32(v):
    if isinstance(v, float):
        return np.float32(v).item()
    if isinstance(v, list):
        return [_f32(x) for x in v]
    return v


def _same_value(a, b):
    """Equality that tells -0.0 from 0.0 and None from an empty list."""
    if isinstance(a, list) and isinstance(b, list):
        return len(a) == len(b) and all(map(_same_value, a, b))
    return type(a) is type(b) and a == b and repr(a) == repr(b)


def assert_equals_host(batch, img, schema, record_type):
    host = cpu_engine.decode_buffer(np.frombuffer(img, np.uint8), schema,
                                    record_type, True)
    assert batch.num_rows == host.num_rows
    assert len(batch.columns) == len(host.columns)
    for f, a, b in zip(schema.fields, batch.columns, host.columns):
        for part in PARTS:
            va, vb = getattr(a, part), getattr(b, part)
            assert (va is None) == (vb is None), (f.name, part)
            if vb is not None:
                va, vb = np.asarray(va), np.asarray(vb)
                assert va.dtype == vb.dtype, (f.name, part)
                assert va.shape == vb.shape, (f.name, part)
                assert va.tobytes() == vb.tobytes(), (f.name, part)
    return host


def head(col, r0, r1):
    """The parts of a column that rows [r0, r1) own, offsets rebased."""
    ro = np.asarray(col.row_off)
    v0, v1 = int(ro[r0]), int(ro[r1])
    out = {"presence": np.asarray(col.presence)[r0:r1],
           "row_off": ro[r0:r1 + 1] - v0}
    vals = np.asarray(col.values)
    if col.elem_off is not None:
        eo = np.asarray(col.elem_off)
        out["elem_off"] = eo[v0:v1 + 1] - eo[v0]
        out["values"] = vals[eo[v0]:eo[v1]]
    else:
        out["values"] = vals[v0:v1]
    if col.list_off is not None:
        lo, so = np.asarray(col.list_off), np.asarray(col.sub_off)
        out["list_off"] = lo[r0:r1 + 1] - lo[r0]
        out["sub_off"] = so[lo[r0]:lo[r1] + 1] - v0
    return out


def assert_same_rows(a, ra, b, rb, n):
    """Rows [ra, ra+n) of batch a are rows [rb, rb+n) of batch b."""
    for ca, cb in zip(a.columns, b.columns):
        ha, hb = head(ca, ra, ra + n), head(cb, rb, rb + n)
        assert ha.keys() == hb.keys()
        for part in ha:
            assert ha[part].dtype == hb[part].dtype, part
            assert ha[part].tobytes() == hb[part].tobytes(), part


# ---------------------------------------------------------------------------
# Malformed records
# ---------------------------------------------------------------------------

OVERLONG = b"\x80" * 11 + b"\x01"


def _malformed_payloads():
    m = {}
    body = packed([1, 2, 3])
    m["list-length-past-record"] = example(entry(
        "ints", b"\x1a" + varint(len(body) + 5) + body))
    m["run-ends-mid-varint"] = example(entry(
        "ints", feature(INT64, ld(1, b"\x05\x80"))))
    m["overlong-varint-short-run"] = example(entry(
        "ints", feature(INT64, ld(1, OVERLONG))))
    long_run = OVERLONG + b"".join(varint(-(i + 1)) for i in range(76))
    assert len(long_run) == 772
    m["overlong-varint-long-run"] = example(entry(
        "ints", feature(INT64, ld(1, long_run))))
    # the same away from lane 0: one byte per lane, and 13 bytes per lane
    # with the over-long varint across the lanes 30 and 31
    ones = b"".join(varint(v) for v in run_of(20, ONES))
    m["overlong-varint-inside-short-run"] = example(entry(
        "ints", feature(INT64, ld(1, ones + OVERLONG + ones))))
    tens = b"".join(varint(-(i + 1)) for i in range(40))
    assert len(tens + OVERLONG + tens) == 812 and 400 // 13 == 30
    m["overlong-varint-inside-long-run"] = example(entry(
        "ints", feature(INT64, ld(1, tens + OVERLONG + tens))))
    m["kind-mismatch"] = example(entry("ints", feature(FLOAT, packed_f([1.0]))))
    m["bad-wire-type-in-bytes-list"] = example(entry(
        "blobs", feature(BYTES, b"\x08\x05")))
    return m


MALFORMED = tuple(_malformed_payloads())
BAD_RECORD = 2


@functools.lru_cache(maxsize=None)
def malformed_image(name, wave):
    good = [example(_ints(run_of(129, WIDTHS)),
                    entry("blobs", feature(BYTES, bytes_list([b"ok" * k]))))
            for k in range(4)]
    payloads = good[:BAD_RECORD] + [_malformed_payloads()[name]] + good[BAD_RECORD:]
    if wave:
        payloads.append(_pad_payload("Example", PAD_KNOWN,
                                     _pad_bytes(payloads))[0])
    img = b"".join(frame(p) for p in payloads)
    assert is_wave(img, len(payloads)) == wave
    return img


# ---------------------------------------------------------------------------
# The oracle, without a GPU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("group", list(GROUPS))
def test_host_codec_decodes_each_image_to_its_intended_values(group, layout):
    img, schema, rt, rows, first = image(group, layout)
    host = cpu_engine.decode_buffer(np.frombuffer(img, np.uint8), schema, rt,
                                    True)
    assert host.num_rows == len(rows)
    names = [name for name, _, _ in GROUPS[group][2]()]
    names = ["pad"] * first + names + ["pad"] * (len(rows) - first - len(names))
    for f, col in zip(schema.fields, host.columns):
        got = rows_of(col)
        for r, want in enumerate(rows):
            assert _same_value(got[r], _f32(want.get(f.name))), \
                (f.name, r, names[r])


@pytest.mark.parametrize("wave", [False, True], ids=["lane", "wave"])
@pytest.mark.parametrize("name", MALFORMED)
def test_host_codec_refuses_each_malformed_image(name, wave):
    img = malformed_image(name, wave)
    # framed with valid CRCs: the frames are found, the decode fails
    off, _ = _native.scan_frames(np.frombuffer(img, np.uint8), True)
    assert len(off) == 5 + wave
    with pytest.raises(RuntimeError, match="decode failed|kind does not match"):
        cpu_engine.decode_buffer(np.frombuffer(img, np.uint8), EXAMPLE_SCHEMA,
                                 "Example", True)
    # and without the damaged record the same image decodes
    payloads = _malformed_payloads()
    rest = img.replace(frame(payloads[name]), b"")
    assert len(rest) == len(img) - len(payloads[name]) - 16
    cpu_engine.decode_buffer(np.frombuffer(rest, np.uint8), EXAMPLE_SCHEMA,
                             "Example", True)


def _varint_starts(vals):
    starts, pos = set(), 0
    for v in vals:
        starts.add(pos)
        pos += len(varint(v))
    return starts, pos


def test_runs_have_the_lane_geometry_they_claim():
    # wave_extract_i64_packed gives lane l bytes [l * chunk, (l + 1) * chunk)
    starts, n = _varint_starts(INSIDE_RUN)
    chunk = -(-n // 64)
    assert (n, chunk) == (761, 12) and chunk % 10
    bounds = [l * chunk for l in range(1, 64) if l * chunk < n]
    assert len(bounds) == 63 and not starts & set(bounds)
    starts, n = _varint_starts(ALIGNED_RUN)
    assert n == 640 and all(l * 10 in starts for l in range(64))
    for src, n in itertools.product(SOURCES, RUN_BYTES):
        vals = run_of(n, SOURCES[src])
        assert all(INT64_MIN <= v <= INT64_MAX for v in vals)
        widths = {len(varint(v)) for v in vals}
        if src == "ones":
            assert widths == {1}
        if src == "tens" and n % 10 == 0:
            assert widths == {10}
        if src == "widths" and n >= 127:
            assert widths == set(range(1, 11))
    # the over-long varint lies in lane 0's bytes of either damaged run
    assert -(-len(OVERLONG) // 64) == 1 and -(-772 // 64) == 13


def test_bytes_elements_cover_every_offset_residue():
    """copy_wave moves u64 words from unaligned addresses and finishes with
    a byte tail: elements long enough for both start at every source and
    destination offset mod 8 (image and column start on aligned addresses)."""
    img, schema, rt, rows, _ = image("bytes", "lane")
    pos, src, dst, at = 0, set(), set(), 0
    for row in rows:
        for e in row["blobs"]:
            if len(e) >= 9:
                i = img.index(e, pos)
                src.add(i % 8)
                dst.add(at % 8)
                pos = i + len(e)
            at += len(e)
    assert src == set(range(8)) and dst == set(range(8))
    seen = {len(e) for row in rows for e in row["blobs"]}
    assert set(ELEM_BYTES) <= seen


def test_size_records_have_the_payload_lengths():
    img = image("sizes", "lane")[0]
    _, lens = _native.scan_frames(np.frombuffer(img, np.uint8), True)
    assert tuple(int(n) for n in lens) == PAYLOAD_BYTES


# ---------------------------------------------------------------------------
# Decode on the GPU
# ---------------------------------------------------------------------------

def _decode(img, schema, rt, verify_crc):
    return _g().decode_buffer_to_cpu(np.frombuffer(img, np.uint8), schema, rt,
                                     verify_crc=verify_crc)


@gpu
@pytest.mark.parametrize("verify_crc", [True, False], ids=["crc", "nocrc"])
@pytest.mark.parametrize("layout", WAVE_LAYOUTS)
@pytest.mark.parametrize("group", list(GROUPS))
def test_wave_and_lane_decode_equal_host_codec(group, layout, verify_crc):
    lane_img, schema, rt, lane_rows, _ = image(group, "lane")
    wave_img, _, _, wave_rows, first = image(group, layout)
    assert not is_wave(lane_img, len(lane_rows))  # per-lane kernels
    assert is_wave(wave_img, len(wave_rows))      # one record per wave
    lane = _decode(lane_img, schema, rt, verify_crc)
    wave = _decode(wave_img, schema, rt, verify_crc)
    assert_equals_host(lane, lane_img, schema, rt)
    assert_equals_host(wave, wave_img, schema, rt)
    assert_same_rows(wave, first, lane, 0, len(lane_rows))


@gpu
@pytest.mark.parametrize("group", ["packed", "bytes", "sequence"])
def test_streamed_read_runs_the_wave_kernels_on_ranges(tmp_path, monkeypatch,
                                                       group):
    g = _g()
    img, schema, rt, rows, first = image(group, "wave-front")
    assert is_wave(img, len(rows))
    path = str(tmp_path / "f.tfrecord")
    with open(path, "wb") as f:
        f.write(img)
    assert _native.file_mmap_pinned(path, len(img), False)[1]
    reads, ranges = [], []

    class Watched(g._StreamedRead):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            reads.append(self)

        def _extract(self, r1, gated):
            ranges.append((self.x_done, r1))
            super()._extract(r1, gated)

    monkeypatch.setattr(g, "_StreamedRead", Watched)
    monkeypatch.setattr(g, "_STREAM_DECODE", True)
    monkeypatch.setattr(g, "_STREAM_EXTRACT", True)
    monkeypatch.setattr(g, "_READ_SLICE", 4 << 10)
    g.last_read.clear()
    batch = g.batch_to_host(
        g.read_file_to_batch_pipelined(path, schema, rt, verify_crc=True))
    assert g.last_read["path"] == "streamed" and g.last_read["slices"] >= 3
    assert len(reads) == 1 and reads[0].avg_bytes > WAVE_BYTES  # wave kernels
    if group != "sequence":  # its records fit one slice
        # the records behind the padding span several slices, so some
        # extraction starts past row 0
        assert any(r0 > 0 for r0, _ in ranges), ranges
    assert_equals_host(batch, img, schema, rt)
    lane_img, _, _, lane_rows, _ = image(group, "lane")
    assert not is_wave(lane_img, len(lane_rows))
    lane = _decode(lane_img, schema, rt, True)
    assert_same_rows(batch, first, lane, 0, len(lane_rows))


def _byte_array_image(wave):
    payloads = [bytes((5 * i + n) % 249 for i in range(n))
                for n in PAYLOAD_BYTES]
    if wave:
        payloads.append(bytes(i % 253 for i in range(_pad_bytes(payloads))))
    img = b"".join(frame(p) for p in payloads)
    assert is_wave(img, len(payloads)) == wave
    # gpu_gather_payloads switches on the payload bytes per record
    assert (sum(map(len, payloads)) // len(payloads) > WAVE_BYTES) == wave
    return img, payloads


@pytest.mark.parametrize("wave", [False, True], ids=["lane", "wave"])
def test_host_codec_decodes_byte_array_image(wave):
    img, payloads = _byte_array_image(wave)
    host = cpu_engine.decode_buffer(np.frombuffer(img, np.uint8),
                                    byte_array_schema(), "ByteArray", True)
    assert rows_of(host.columns[0]) == [[p] for p in payloads]


@gpu
@pytest.mark.parametrize("verify_crc", [True, False], ids=["crc", "nocrc"])
@pytest.mark.parametrize("wave", [False, True], ids=["lane", "wave"])
def test_byte_array_decode_equals_host_codec(wave, verify_crc):
    img, payloads = _byte_array_image(wave)
    assert is_wave(img, len(payloads)) == wave
    out = _decode(img, byte_array_schema(), "ByteArray", verify_crc)
    assert_equals_host(out, img, byte_array_schema(), "ByteArray")


def _flips(img):
    """name -> (byte offsets to damage, lowest damaged record)."""
    off, lens = _native.scan_frames(np.frombuffer(img, np.uint8), True)
    off, lens = [int(o) for o in off], [int(n) for n in lens]
    r65, r4097, r64 = (lens.index(n) for n in (65, 4097, 64))
    return {
        "first-byte-of-65": ([off[r65]], r65),
        "last-byte-of-4097": ([off[r4097] + 4096], r4097),
        "length-header": ([off[r64] - 12], r64),
        "length-crc": ([off[r64] - 2], r64),
        "two-records": ([off[r4097] + 2000, off[r65] + 64], min(r65, r4097)),
    }


FLIPS = ("first-byte-of-65", "last-byte-of-4097", "length-header",
         "length-crc", "two-records")


def _flip_image(fmt, wave):
    if fmt == "ByteArray":
        return _byte_array_image(wave)[0], byte_array_schema()
    img, schema, _, _, _ = image("sizes", "wave-known" if wave else "lane")
    return img, schema


@pytest.mark.parametrize("fmt", ["Example", "ByteArray"])
@pytest.mark.parametrize("flip", FLIPS)
def test_host_codec_reports_each_flipped_bit(fmt, flip):
    img, schema = _flip_image(fmt, True)
    bad = bytearray(img)
    for at in _flips(img)[flip][0]:
        bad[at] ^= 0x10
    with pytest.raises(RuntimeError, match="CRC"):
        cpu_engine.decode_buffer(np.frombuffer(bytes(bad), np.uint8), schema,
                                 fmt, True)


@gpu
@pytest.mark.parametrize("wave", [False, True], ids=["lane", "wave"])
@pytest.mark.parametrize("fmt", ["Example", "ByteArray"])
@pytest.mark.parametrize("flip", FLIPS)
def test_flipped_bit_names_the_lowest_damaged_record(flip, fmt, wave):
    import torch
    g = _g()
    img, schema = _flip_image(fmt, wave)
    # the frames as they were before the damage: a damaged length must be
    # caught by the kernels' own length-CRC check, not by frame discovery
    off, lens = _native.scan_frames(np.frombuffer(img, np.uint8), True)
    assert is_wave(img, len(off)) == wave
    places, record = _flips(img)[flip]
    bad = bytearray(img)
    for at in places:
        bad[at] ^= 0x10
    data = torch.frombuffer(bad, dtype=torch.uint8).cuda()
    off_d = torch.from_numpy(np.asarray(off, np.int64)).cuda()
    len_d = torch.from_numpy(np.asarray(lens, np.int64)).cuda()
    with pytest.raises(RuntimeError) as e:
        g.decode_device(data, off_d, len_d, schema, fmt, True)
    assert str(e.value) == f"corrupt TFRecord: bad CRC in record {record}"
    if flip in ("first-byte-of-65", "last-byte-of-4097", "two-records"):
        with pytest.raises(RuntimeError) as e:
            _decode(bytes(bad), schema, fmt, True)
        assert str(e.value) == f"corrupt TFRecord: bad CRC in record {record}"


@gpu
@pytest.mark.parametrize("verify_crc", [True, False], ids=["crc", "nocrc"])
@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_record_fails_in_wave_mode_as_in_lane_mode(name, verify_crc):
    lane_img, wave_img = malformed_image(name, False), malformed_image(name, True)
    assert not is_wave(lane_img, 5) and is_wave(wave_img, 6)
    with pytest.raises(Exception) as lane:
        _decode(lane_img, EXAMPLE_SCHEMA, "Example", verify_crc)
    with pytest.raises(Exception) as wave:
        _decode(wave_img, EXAMPLE_SCHEMA, "Example", verify_crc)
    assert type(lane.value) is RuntimeError
    assert f"record {BAD_RECORD}" in str(lane.value)
    assert type(wave.value) is type(lane.value)
    assert str(wave.value) == str(lane.value)


# ---------------------------------------------------------------------------
# Emit
# ---------------------------------------------------------------------------

def _emit_rows(record_type):
    """{field: one value per row}: the shapes of the decode cases."""
    rng = np.random.default_rng(31)
    elems = [rng.bytes(n) for n in ELEM_BYTES]
    if record_type == "Example":
        return EXAMPLE_SCHEMA, {
            "ints": [[], [INT64_MIN], run_of(100, WIDTHS)[:63],
                     (WIDTHS * 4)[:64], (EXTREMES * 17)[:65], None,
                     (WIDTHS * 7)[:130], run_of(129, ONES)],
            "flts": [None, [], [1.5], _quarter(130), None, [-0.0], [],
                     _quarter(65, 3)],
            "blobs": [None, [], elems, [b""], elems[::-1], [b"", b""],
                      elems[3:] + elems[:3], None],
        }
    return SEQUENCE_SCHEMA, {
        "ctx": [[], None, (WIDTHS * 4)[:65], [1], [INT64_MAX]],
        "sids": [[[], [1, -1], []], [], None,
                 [(WIDTHS * 7)[:130], [], (EXTREMES * 16)[:63], [0]],
                 [[], []]],
        "sflts": [None, [[]], [_quarter(64), [], [2.5]], [], [[0.5], []]],
        "sblobs": [[[]], None, [elems[:6], [], elems[6:]], [[b""], []], []],
    }


def _emit_batch(record_type, wave):
    schema, columns = _emit_rows(record_type)
    n = len(next(iter(columns.values())))
    columns = dict(columns)
    columns[PAD_KNOWN] = [None] * n
    if wave:
        for name in columns:
            columns[name] = columns[name] + [None]
        columns[PAD_KNOWN][-1] = bytes(i % 253 for i in range(
            (n + 1) * (WAVE_BYTES + 96)))
        n += 1
    cols = [column_from_values(columns[f.name], f.dataType, True, f.name)
            for f in schema.fields]
    return RecordBatch(schema, cols, n), columns


@pytest.mark.parametrize("wave", [False, True], ids=["lane", "wave"])
@pytest.mark.parametrize("record_type", ["Example", "SequenceExample"])
def test_host_encoded_emit_batch_decodes_back(record_type, wave):
    batch, columns = _emit_batch(record_type, wave)
    img = cpu_engine.encode_batch(batch, record_type)
    assert is_wave(img, batch.num_rows) == wave
    host = cpu_engine.decode_buffer(np.frombuffer(img, np.uint8), batch.schema,
                                    record_type, True)
    for f, col in zip(batch.schema.fields, host.columns):
        want = columns[f.name]
        if f.name == PAD_KNOWN:
            want = [None if v is None else [v] for v in want]
        got = rows_of(col)
        assert len(got) == len(want)
        for r, (a, b) in enumerate(zip(got, want)):
            assert _same_value(a, _f32(b)), (f.name, r)


@gpu
@pytest.mark.parametrize("wave", [False, True], ids=["lane", "wave"])
@pytest.mark.parametrize("record_type", ["Example", "SequenceExample"])
def test_emit_equals_host_codec(tmp_path, record_type, wave):
    g = _g()
    batch, _ = _emit_batch(record_type, wave)
    want = cpu_engine.encode_batch(batch, record_type)
    assert is_wave(want, batch.num_rows) == wave
    dev = g.batch_to_device(batch)
    assert g.device_to_bytes(g.encode_device(dev, record_type)) == want
    # five slices over the rows: every launch but the first starts at r0 > 0
    path = str(tmp_path / "emit.tfrecord")
    assert g.write_batch_to_file(dev, path, record_type, slices=5) == len(want)
    assert _native.file_mmap_pinned(path, len(want), False)[1]
    with open(path, "rb") as f:
        assert f.read() == want


def _byte_array_batch(wave):
    _, payloads = _byte_array_image(wave)
    elem_off = np.zeros(len(payloads) + 1, np.int64)
    np.cumsum([len(p) for p in payloads], out=elem_off[1:])
    col = WireColumn(kind=BYTES, is_seq=False,
                     presence=np.ones(len(payloads), np.uint8),
                     row_off=np.arange(len(payloads) + 1, dtype=np.int64),
                     values=np.frombuffer(b"".join(payloads), np.uint8).copy(),
                     elem_off=elem_off)
    return RecordBatch(byte_array_schema(), [col], len(payloads))


@pytest.mark.parametrize("wave", [False, True], ids=["lane", "wave"])
def test_host_codec_frames_byte_arrays_like_the_builder(wave):
    assert (cpu_engine.encode_batch(_byte_array_batch(wave), "ByteArray")
            == _byte_array_image(wave)[0])


@gpu
@pytest.mark.parametrize("wave", [False, True], ids=["lane", "wave"])
def test_byte_array_framing_equals_host_codec(tmp_path, wave):
    g = _g()
    batch = _byte_array_batch(wave)
    want = cpu_engine.encode_batch(batch, "ByteArray")
    assert is_wave(want, batch.num_rows) == wave
    dev = g.batch_to_device(batch)
    assert g.device_to_bytes(g.encode_device(dev, "ByteArray")) == want
    path = str(tmp_path / "ba.tfrecord")
    assert g.write_batch_to_file(dev, path, "ByteArray") == len(want)
    with open(path, "rb") as f:
        assert f.read() == want
