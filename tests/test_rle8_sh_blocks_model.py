"""The Python builder and splitter of the rle8_sh block container (tests/rle8_sh_blocks_testlib.py) against each other and, where the compiled
reference is present (oracle/_ref/libhsrle_ref.so), against it: every block stream of a built container is the reference's stream of that block's
bytes, and the reference's decoder gives the block back."""
import struct

import pytest

import rle8_sh_blocks_testlib as B
import rle8_sh_testlib as T
from mmtf_testlib import video_shaped


def inputs():
    c = T.input_set()
    return {
        "members_3_blocks": (c["alphabet4_1000"] + c["raw_263"] + c["r_rich_417_encoded"] + c["change_10_then_r"])[: 3 * 128 + 17],
        "one_byte": b"\x7F",
        "one_block": c["alphabet3_1000"][:128],
        "one_block_and_a_byte": c["alphabet3_1000"][:129],
        "short_coded_stretches": T.short_coded_stretches(2 * 1152 + 5),
        "r_rich": T.r_rich(3000, 4, 3),
        "video": video_shaped(3 * 4096 + 17),
        "noise": T.noise(1000, 4),
    }


CASES = [(name, bs) for name in inputs() for bs in (128, 1152, 4096)]


@pytest.mark.parametrize("name,bs", CASES)
def test_build_and_split_round_trip(name, bs):
    data = inputs()[name]
    c = B.build(data, bs)
    h, streams = B.split(c)
    assert (h["uncompressedSize"], h["blockSize"], h["blockCount"]) == (len(data), bs, B.block_count(len(data), bs))
    assert len(c) == h["totalSize"] <= B.bound(len(data), bs)
    assert streams == [T.model_compress(b)[0] for b in B.blocks_of(data, bs)]
    for s, b in zip(streams, B.blocks_of(data, bs)):
        assert struct.unpack_from("<II", s, 0) == (len(b), len(s))                          # every block stream has its own 8-byte header
    assert B.decode(c) == data
    assert B.from_streams(streams, len(data), bs) == c


def test_split_sees_a_cut_stream():
    data = inputs()["members_3_blocks"]
    _, streams = B.split(B.build(data, 128))
    streams[1] = streams[1][:-1]
    assert B.decode(B.from_streams(streams, len(data), 128)) is None


@pytest.mark.skipif(not T.Rle8ShReference.available(), reason="the compiled reference is not built")
@pytest.mark.parametrize("name,bs", CASES)
def test_block_streams_are_the_references(name, bs):
    ref = T.Rle8ShReference()
    data = inputs()[name]
    _, streams = B.split(B.build(data, bs))
    for i, (s, b) in enumerate(zip(streams, B.blocks_of(data, bs))):
        assert s == ref.compress(b), f"{name} block {i}"
        assert ref.decompress(s, len(b)) == (len(b), b), f"{name} block {i}"
