"""CPU tests of the LZ4 codec: the decoder core (csrc/lz4_core.h) through
`_native.host_unlz4_block`, in place and through the kernel's staging
window, against pyarrow's `lz4_raw` decode of the same bytes, and the
`.lz4` container through the CPU engine. tests/test_gpu_lz4.py runs the
same cases on the device."""

import struct

import numpy as np
import pyarrow as pa
import pytest

import spark_tfrecord_amd as stf
from spark_tfrecord_amd import _native
from spark_tfrecord_amd.io import paths as P

LIB = pa.Codec("lz4_raw")
_rng = np.random.default_rng(4)


def R(n):
    return _rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def seq(literals, offset=None, match_len=0):
    """One LZ4 sequence; offset None = a block's last one, literals only."""
    def ext(n):  # the length bytes behind a nibble of 15
        return b"" if n < 15 else b"\xff" * ((n - 15) // 255) + bytes([(n - 15) % 255])
    m = 0 if offset is None else match_len - 4
    out = bytes([min(len(literals), 15) << 4 | min(m, 15)]) + ext(len(literals)) + literals
    return out if offset is None else out + struct.pack("<H", offset) + ext(m)


TAIL = (b"the-last-12b", None, 0)  # the format's end-of-block rules, kept


def block(*seqs):
    """(raw LZ4 block, bytes it produces) of (literals, offset, match_len)s."""
    seqs += (TAIL,)
    return b"".join(seq(*s) for s in seqs), sum(len(s[0]) + s[2] for s in seqs)


def upto(t):
    """Sequences of exactly t bytes (4038..4292): the next token is byte t."""
    return (R(4000), 5, 4), (R(t - 4023), 5, 4)


TEXT = b"".join(b"row-%d,name=%d;" % (i, i % 7) for i in range(4000))
VALID = {f"literal_{n}": block((R(20), 7, 5), (R(n), 9, 6)) for n in (0, 14, 15, 270, 271)}
VALID.update({f"match_{n}": block((R(40), 33, n)) for n in (4, 18, 19, 274, 5000)})
VALID.update({f"offset_{o}": block((R(200), o, 100)) for o in (1, 2, 7, 8, 100, 99)})
VALID.update({
    "offset_65535": block((R(65535), 65535, 20)),
    "literals_only": (seq(R(1000)), 1000),
    "lib_text": (LIB.compress(TEXT, asbytes=True), len(TEXT)),
    "lib_random": (LIB.compress(R(3000), asbytes=True), 3000),
    # the staging window (4096 bytes): its edge inside each kind of header
    "token_on_window_end": block(*upto(4095), (R(9), 30, 8)),
    "length_bytes_over_refill": block(*upto(4094), (R(273), 30, 8)),
    "offset_over_refill": block(*upto(4091), (R(3), 30, 8)),
    "literal_over_window": block((R(30), 3, 9), (R(5000), 4000, 70), (R(6), 1, 300)),
})
# pyarrow decodes every valid case: its bytes are the expectation
VALID = {k: (c, LIB.decompress(c, decompressed_size=n, asbytes=True)) for k, (c, n) in VALID.items()}

_L = b"lz4-block-hdr"
_N = 13 + 20 + 12
BAD = {  # name: (block, cap, cause)
    "offset_zero": (block((_L, 0, 20))[0], _N, 1),
    "offset_before_block": (block((_L, 14, 20))[0], _N, 2),
    "length_bytes_cut": (b"\xf0\xff\xff", _N, 3),
    "literal_cut": (seq(_L)[:-1], _N, 4),
    "output_overrun": (block((_L, 7, 30))[0], _N, 5),
    "no_last_sequence": (seq(_L, 7, 20), _N, 6),
    "input_left": (block((_L, 7, 20))[0] + b"\x00\x00\x00", _N, 7),
}


def one_block_file(comp, raw_len):
    return struct.pack(">II", raw_len, len(comp)) + comp


def container_files():
    """{name: (file image, bytes it holds)}"""
    a, b, c = (VALID[k] for k in ("lib_text", "offset_7", "literal_271"))
    three = struct.pack(">I", sum(len(x[1]) for x in (a, b, c))) + b"".join(
        struct.pack(">I", len(x[0])) + x[0] for x in (a, b, c))
    odd = one_block_file(seq(b"odd"), 3)  # 12 bytes: what follows sits odd
    return {"three_chunks": (three + one_block_file(b[0], len(b[1])), a[1] + b[1] + c[1] + b[1]),
            "odd_offset": (odd + one_block_file(a[0], len(a[1])), b"odd" + a[1]),
            "empty": (b"", b""),
            "terminator": (one_block_file(b[0], len(b[1])) + bytes(4) + b"junk", b[1])}


def _cause(comp, cap, window):
    with pytest.raises(RuntimeError, match=r"cause \d+$") as e:
        _native.host_unlz4_block(comp, cap, window)
    return int(str(e.value).rsplit(" ", 1)[1])


@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("name", VALID)
def test_block(name, window):
    comp, want = VALID[name]
    assert _native.host_unlz4_block(comp, len(want), window) == want
    assert _native.host_unlz4_block(comp, len(want) + 77, window) == want
    assert _cause(comp[:-1], len(want), window) in (4, 6)


@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("name", BAD)
def test_malformed_block(tmp_path, name, window):
    comp, cap, cause = BAD[name]
    assert _cause(comp, cap, window) == cause  # the binding checks its guards
    p = tmp_path / "bad.tfrecord.lz4"
    p.write_bytes(one_block_file(comp, cap))
    with pytest.raises(ValueError, match="lz4"):
        P.decompress_file(str(p))


@pytest.mark.parametrize("name", container_files())
def test_container(tmp_path, name):
    img, want = container_files()[name]
    p = tmp_path / f"{name}.tfrecord.lz4"
    p.write_bytes(img)
    assert P.decompress_file(str(p)) == want
    rows, total, device_ok = P.lz4_walk(img, name)
    assert device_ok and total == len(want)
    assert [r[3] for r in rows] == [struct.unpack_from(">I", img, r[0] - 4)[0] for r in rows]


@pytest.mark.parametrize("codec", ["lz4", "org.apache.hadoop.io.compress.Lz4Codec"])
def test_file_round_trip(tmp_path, codec):
    rows = {"x": np.arange(5000, dtype=np.int64), "s": [f"row-{i % 13}" for i in range(5000)]}
    d = str(tmp_path / "out")
    stf.write_tfrecord(rows, d, codec=codec, engine="cpu")
    files = P.list_data_files(d)
    assert files and all(f.endswith(".tfrecord.lz4") for f in files)
    assert P.normalize_codec(codec) == "lz4" == P.codec_from_path(files[0])
    got = sorted((r["x"], r["s"]) for r in stf.read_tfrecord(d, engine="cpu").collect())
    assert got == sorted(zip(rows["x"].tolist(), rows["s"]))
