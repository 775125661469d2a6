"""The rle8_mmtf128 block container built in plain Python (rle8_mmtf_blocks_testlib.py): it splits back into streams the model decoder reads, its bound
holds where a block needs the most, and -- where the compiled reference is built -- every block stream is the reference's stream of the block's bytes.
The GPU tests compare the library with this container."""
import random

import pytest

import rle8_mmtf_blocks_testlib as B
import rle8_mmtf_testlib as T
from mmtf_testlib import video_shaped

needs_reference = pytest.mark.skipif(not T.Rle8MmtfReference.available(), reason="oracle/_ref/libhsrle_ref.so is not built")

BLOCK_SIZES = (128, 1152, 4096)


def inputs(bs):
    rng = random.Random(bs)
    return {
        "alphabet3": T.random_alphabet(3 * bs + 17, 3, 2, run=2),
        "alphabet256": T.random_alphabet(2 * bs + 5, 256, 3),
        "video": video_shaped(4 * bs - 9),
        "zeros": bytes(2 * bs + 1),
        "short": rng.randbytes(15),
        "one_block": T.random_alphabet(bs, 5, 4),
    }


def deterministic_blocks(bs, blocks=5):
    """Every block begins with 16 random, not all equal bytes, one of them >= 16: from identity lists row 0's ranks are the bytes themselves, so the
    reference's undefined start value cannot change any block's stream."""
    rng = random.Random(bs + 1)
    out = bytearray()
    for i in range(blocks):
        row = bytearray(rng.randbytes(16))
        row[0], row[1] = 200, 3
        out += row + T.random_alphabet(bs - 16, 3, i, run=2)
    return bytes(out)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_split_of_build_round_trips_through_the_model_decoder(bs):
    for name, data in inputs(bs).items():
        c = B.build(data, bs)
        h, streams = B.split(c)
        assert (h["uncompressedSize"], h["blockSize"], h["blockCount"]) == (len(data), bs, B.block_count(len(data), bs)), name
        for s, block in zip(streams, B.blocks_of(data, bs)):
            assert T.model_decompress(s) == block, name
        assert B.decode(c) == data, name
        assert len(c) <= B.bound(len(data), bs), name


def test_the_bound_is_met_by_incompressible_blocks():
    """A block of >= 32 literal 8 bit rows is one COPY with a 4-byte header: its bytes + 8 (stream header) + 4 + 1 (the terminator) = bytes + 13."""
    for bs in (1152, 4096):
        rows = bs // 16
        data = B.data_from_block_specs([[("copy", rows, 255)]] * 3, bs)
        c = B.build(data, bs)
        _, streams = B.split(c)
        assert [len(s) for s in streams] == [bs + 13] * 3
        assert len(c) == B.bound(len(data), bs)
    # under 32 rows the COPY header is one byte: the bound has slack
    data = B.data_from_block_specs([[("copy", 8, 255)]] * 2, 128)
    assert len(B.build(data, 128)) == B.bound(256, 128) - 2 * 3
    assert B.bound(1, 0) == B.bound(1, 4096) == 64 + 16 + 1 + 13 + 32
    assert B.bound(0, 128) == 0 and B.bound(128, 64) == 0 and B.bound(128, 192) == 0 and B.bound(128 << 32, 128) == 0


@pytest.fixture(scope="module")
def ref():
    return T.Rle8MmtfReference()


def check_against_reference(ref, data, bs):
    """Number of blocks whose stream was compared byte for byte."""
    _, streams = B.split(B.build(data, bs))
    exact = 0
    for i, (mine, block) in enumerate(zip(streams, B.blocks_of(data, bs))):
        theirs = ref.compress(block)
        if T.reference_is_deterministic(block):
            assert mine == theirs, i
            exact += 1
        else:
            assert mine[T.first_copy_end(mine) :] == theirs[T.first_copy_end(theirs) :], i
        assert ref.decompress(mine, len(block)) == (len(block), block), i
    return exact


@needs_reference
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_every_block_stream_is_the_references(ref, bs):
    for name, data in inputs(bs).items():
        check_against_reference(ref, data, bs)


@needs_reference
@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_blocks_that_leave_the_reference_no_choice_are_equal_byte_for_byte(ref, bs):
    data = deterministic_blocks(bs)
    assert all(T.reference_is_deterministic(b) for b in B.blocks_of(data, bs))
    assert check_against_reference(ref, data, bs) == 5                       # the byte-for-byte branch, for every block
