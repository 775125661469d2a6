"""The sequential model of rle8_mmtf128 (rle8_mmtf_testlib.py) against the compiled reference (skipped where it is absent) and against the stored
vectors minted from it (tests/golden/rle8_mmtf/vectors.json).  The GPU tests compare the library with this model."""
import json
import random

import pytest

import rle8_mmtf_testlib as T
from mmtf_testlib import every_symbol_per_column, mmtf_enc, video_shaped

needs_reference = pytest.mark.skipif(not T.Rle8MmtfReference.available(), reason="oracle/_ref/libhsrle_ref.so is not built")

ALPHABETS = (1, 2, 3, 5, 17, 256)
SIZES = (1, 15, 16, 17, 100, 16 * 40 + 3, 4096, 5000)


def inputs():
    out = []
    for a in ALPHABETS:
        for n in SIZES:
            out.append((f"alphabet{a}_{n}", T.random_alphabet(n, a, 1)))
    out.append(("every_symbol", every_symbol_per_column(16 * 300 + 7, 16)))
    out.append(("video", video_shaped(6000)))
    rng = random.Random(5)
    out.append(("literal_high", T.data_from_rank_rows(T.literal_rows(40, 200, rng), b"\x01\x02")))
    out.append(("literal_then_runs", T.data_from_rank_rows(T.rows_from_spec([("copy", 3, 77), ("rle", 130, 0), ("rle", 2, 9), ("copy", 33, 3)]))))
    return out


INPUTS = inputs()


@pytest.fixture(scope="module")
def ref():
    return T.Rle8MmtfReference()


@needs_reference
def test_bounds_are_the_references(ref):
    for n in (0, 1, 1000, 1 << 30, (1 << 30) + 1):
        want = 0 if n > 1 << 30 else n + 8
        assert ref.bounds(n) == want and ref.bounds(n, "rle8_mmtf256_compress_bounds") == want


@needs_reference
@pytest.mark.parametrize("name,data", INPUTS, ids=[i[0] for i in INPUTS])
def test_model_against_reference(ref, name, data):
    mine, theirs = T.model_compress(data), ref.compress(data)
    assert len(theirs) >= 10
    if T.reference_is_deterministic(data):
        assert mine == theirs
    else:
        # the reference's first packet may be wider than its rows need (undefined start value): equal behind it
        a, b = T.first_copy_end(mine), T.first_copy_end(theirs)
        assert mine[a:] == theirs[b:]
        assert T.structure(T.parse_stream(mine)[1]) == T.structure(T.parse_stream(theirs)[1])
    assert ref.decompress(mine, len(data)) == (len(data), data)
    assert T.model_decompress(theirs) == data
    assert T.model_decompress(mine) == data


@needs_reference
@pytest.mark.parametrize("alphabet", ALPHABETS)
def test_local_packet_rule_against_reference(ref, alphabet):
    """Maximal runs, a null COPY between adjacent RLE packets, a first COPY always, the two endings: nothing depends on carried state."""
    for seed in range(12):
        n = random.Random(seed).choice((16, 160, 1600, 3000, 4099))
        data = T.random_alphabet(n, alphabet, seed + 10, run=1 + seed % 3)
        want = T.local_rule_packets(mmtf_enc(data, 16))
        assert T.structure(T.parse_stream(ref.compress(data))[1]) == want
        assert T.structure(T.parse_stream(T.model_compress(data))[1]) == want


def test_model_local_rule_without_reference():
    for alphabet in ALPHABETS:
        data = T.random_alphabet(2500, alphabet, 3)
        assert T.structure(T.parse_stream(T.model_compress(data))[1]) == T.local_rule_packets(mmtf_enc(data, 16))


def golden():
    with open(T.GOLDEN) as f:
        return json.load(f)["vectors"]


def test_golden_vectors():
    """The reference's streams are snapshots (their first width may be arbitrary, they are legal streams all the same): the model decodes them, and
    its own stream equals the snapshot wherever the reference is deterministic, and behind the first COPY packet everywhere."""
    vectors = golden()
    assert len(vectors) >= 20
    for v in vectors:
        data, theirs = bytes.fromhex(v["input"]), bytes.fromhex(v["stream"])
        assert T.model_decompress(theirs) == data, v["name"]
        mine = T.model_compress(data)
        assert T.model_decompress(mine) == data, v["name"]
        if T.reference_is_deterministic(data):
            assert mine == theirs, v["name"]
        else:
            assert mine[T.first_copy_end(mine) :] == theirs[T.first_copy_end(theirs) :], v["name"]


def test_pack_unpack_every_width_and_count():
    rng = random.Random(2)
    for code, top in ((0, 255), (1, 15), (2, 7), (3, 3)):
        for c in range(0, 14):
            rows = T.literal_rows(c, top, rng)
            assert T.unpack_rows(T.pack_rows(rows, code), c, code) == rows


def test_parser_rejects_what_the_library_rejects():
    rows = T.literal_rows(3, 200, random.Random(1))
    good = T.write_stream(48, [("copy", rows, 0, False), ("rle", 0, None, False)])
    assert T.model_decompress(good) == T.data_from_rank_rows(rows)
    assert T.model_decompress(T.write_stream(48, [("copy", rows, 0, False), ("rle", 0, None, False)], stream_size=8 + 1 + 40)) is None     # body past streamSize
    assert T.model_decompress(T.write_stream(32, [("copy", rows, 0, False), ("rle", 0, None, False)])) is None                            # rows past R
    assert T.model_decompress(T.write_stream(48, [("copy", rows, 0, False)])) is None                                                    # no terminator
    assert T.model_decompress(T.write_stream(64, [("copy", rows, 0, False), ("rle", 0, None, False)])) is None                            # rows left over


def test_span_algebra_of_the_kernels_equals_the_model():
    """tools/rle8_mmtf_span_model.py states the encoder's three passes (per-span tables, the two sweeps with their hand-over, emission by the span of a
    group's first row) on the CPU: the same bytes as the sequential model for every span length and cut of the scan."""
    import os
    import sys

    sys.path.insert(0, os.path.join(T.REPO, "tools"))
    import rle8_mmtf_span_model as S

    specs = [[("rle", 61, 0), ("copy", 70, 3), ("rle", 3, 2), ("copy", 200, 3)], [("rle", 59, 1), ("copy", 77, 7), ("rle", 130, 0), ("copy", 9, 7), ("rle", 1, 3)],
             [("copy", 63, 15), ("rle", 1, 0), ("copy", 129, 15), ("rle", 64, 4)], [("rle", 1, 0), ("rle", 1, 1), ("rle", 2, 0), ("rle", 5, 200)],
             [("copy", 2, 3), ("rle", 700, 0), ("copy", 300, 15), ("rle", 1, 7)]]
    datas = [T.data_from_rank_rows(T.rows_from_spec(s), b"\x01\x02") for s in specs] + [T.random_alphabet(3000, a, 9, run=2) for a in (1, 3, 256)] + [bytes(5), bytes(16)]
    for data in datas:
        want = T.model_compress(data)
        for SP, threads in ((64, 1024), (63, 4), (7, 3), (1, 2)):
            assert S.compress(data, SP, threads) == want, (len(data), SP, threads)
