"""CPU tests of the raw-Snappy chunk decoder core (csrc/snappy_core.h)
through its host build, _native.host_unsnap_chunk: the same code the gfx950
kernel runs, the lanes' share of every copy done by a loop."""

import pyarrow as pa
import pytest

import snappy_cases as C
from spark_tfrecord_amd import _native

LIBRARY = C.library_chunks()
HAND = C.hand_chunks()
MALFORMED = C.malformed_chunks()


@pytest.mark.parametrize("name,comp,want", LIBRARY + HAND,
                         ids=[c[0] for c in LIBRARY + HAND])
def test_valid_chunk(name, comp, want):
    got = _native.host_unsnap_chunk(comp, len(want))
    assert got == want
    assert _native.host_unsnap_chunk(comp, len(want)) == got  # deterministic


@pytest.mark.parametrize("name,comp,want", LIBRARY + HAND,
                         ids=[c[0] for c in LIBRARY + HAND])
def test_library_agrees(name, comp, want):
    """The library decodes every case to the same bytes, the hand-assembled
    ones included: they are unusual encodings, not a private dialect."""
    lib = pa.Codec("snappy").decompress(comp, decompressed_size=len(want),
                                        asbytes=True)
    assert lib == want == _native.host_unsnap_chunk(comp, len(want))


@pytest.mark.parametrize("name,comp,expect_len,cause", MALFORMED,
                         ids=[c[0] for c in MALFORMED])
def test_malformed_chunk(name, comp, expect_len, cause):
    with pytest.raises(RuntimeError, match=rf"cause {cause}$"):
        _native.host_unsnap_chunk(comp, expect_len)


def test_one_cause_per_refusal():
    assert sorted(c[3] for c in MALFORMED) == list(range(1, 10))


@pytest.mark.parametrize("name,comp,want", LIBRARY + HAND,
                         ids=[c[0] for c in LIBRARY + HAND])
def test_every_truncation_is_refused(name, comp, want):
    """Cutting a valid chunk anywhere must end in a cause code (the
    sanitizer build of csrc/tests/snappy_selftest.cpp checks the bounds)."""
    step = max(1, len(comp) // 40)
    for cut in range(0, len(comp), step):
        with pytest.raises(RuntimeError, match="cause"):
            _native.host_unsnap_chunk(comp[:cut], len(want))


def test_wrong_expect_len_is_a_mismatch():
    name, comp, want = LIBRARY[3]
    for n in (len(want) - 1, len(want) + 1, 0):
        with pytest.raises(RuntimeError, match="cause 2$"):
            _native.host_unsnap_chunk(comp, n)
    with pytest.raises(ValueError):
        _native.host_unsnap_chunk(comp, -1)
