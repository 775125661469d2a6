"""rle8_mmtf128 on the GPU (csrc/hsrle_rle8mmtf.hip.h) against the sequential model (tests/rle8_mmtf_testlib.py, itself held against the compiled
reference by test_rle8_mmtf_model.py).  Encode: the stream equals the model's byte for byte.  Decode: the model's, the stored reference's and
grammar-written streams (with what no encoder writes) give the model's bytes.  The inputs are made from the PACKETS they shall produce (the inverse
mmtf of chosen rank rows), so every header form, width, group remainder and edge is hit by name.  Malformed streams are refused by the walk's bounds
checks before anything is written."""
import json
import random
import struct

import numpy as np
import pytest

import rle8_mmtf_testlib as T
from mmtf_testlib import every_symbol_per_column, video_shaped

pytestmark = pytest.mark.gpu

GUARD = 4096
DONE, MALFORMED, CAPACITY = 0, 1, 2
_MODEL = {}


def model_stream(data):
    if data not in _MODEL:
        _MODEL[data] = T.model_compress(data)
    return _MODEL[data]


def from_spec(spec, tail=b"", seed=1):
    return T.data_from_rank_rows(T.rows_from_spec(spec, seed), tail)


def cases():
    rng = random.Random(9)
    c = {}
    for n in (1, 15, 16, 17):
        c[f"zeros_{n}"] = bytes(n)
        c[f"random_{n}"] = rng.randbytes(n)
    c["copy_31_32"] = from_spec([("copy", 31, 200), ("rle", 1, 0), ("copy", 32, 200), ("rle", 2, 1), ("copy", 31, 3), ("rle", 1, 0), ("copy", 32, 7)], b"\x05")
    c["rle_127_128"] = from_spec([("rle", 127, 0), ("rle", 128, 1), ("copy", 1, 9), ("rle", 128, 0), ("rle", 127, 3)])
    for top, name, counts in ((3, "2bit", (3, 4, 5)), (7, "3bit", (5, 6, 7)), (15, "4bit", (1, 2, 3)), (255, "8bit", (1, 2))):
        for k in counts:
            c[f"{name}_{k}_rows"] = from_spec([("copy", k, top), ("rle", 1, 0), ("copy", k, top), ("rle", 3, 2)], b"\x01\x00", seed=k)
            c[f"{name}_{k}_rows_last"] = from_spec([("rle", 2, 1), ("copy", k, top)], seed=k + 50)
    # packets that begin in one span of 64 rows and end in another; groups of 4 / 6 / 2 rows across the edge; edges at rows 63, 64, 65
    c["span_edge_2bit"] = from_spec([("rle", 61, 0), ("copy", 70, 3), ("rle", 3, 2), ("copy", 200, 3)])
    c["span_edge_3bit"] = from_spec([("rle", 59, 1), ("copy", 77, 7), ("rle", 130, 0), ("copy", 9, 7), ("rle", 1, 3)], b"\x02" * 15)
    c["span_edge_4bit"] = from_spec([("copy", 63, 15), ("rle", 1, 0), ("copy", 129, 15), ("rle", 64, 4)])
    c["span_edge_8bit"] = from_spec([("copy", 65, 255), ("rle", 63, 0), ("copy", 64, 100)])
    c["edges_63_64_65"] = from_spec([("rle", 63, 0), ("rle", 1, 1), ("rle", 1, 2), ("copy", 63, 3), ("rle", 1, 0), ("copy", 64, 7), ("rle", 65, 9)])
    c["long_rle_many_spans"] = from_spec([("copy", 2, 3), ("rle", 700, 0), ("copy", 300, 15), ("rle", 1, 7)])
    c["adjacent_rles"] = from_spec([("rle", 1, 0), ("rle", 1, 1), ("rle", 2, 0), ("rle", 5, 200), ("rle", 1, 255)], b"\x00")
    c["row0_uniform_ends_with_copy"] = from_spec([("rle", 3, 0), ("copy", 2, 40)])
    c["row0_literal_ends_with_rle"] = from_spec([("copy", 2, 40), ("rle", 3, 0)])
    c["every_symbol_per_column"] = every_symbol_per_column(16 * 520 + 3, 16)                # an RLE row of every rank up to 255
    c["alphabet3_70000"] = T.random_alphabet(70000, 3, 4, run=3)                            # many mmtf segments at the library's segment length
    c["video_70000"] = video_shaped(70000)
    c["alphabet256_5000"] = T.random_alphabet(5000, 256, 5)
    return c


CASES = cases()
SMALL = [k for k, v in CASES.items() if len(v) <= 9000]


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    hsrle.mmtf_tuning(0)
    hsrle.rle8_mmtf_tuning(0)
    yield hsrle
    hsrle.mmtf_tuning(0)
    hsrle.rle8_mmtf_tuning(0)


@pytest.fixture
def tuned(hs):
    yield hs
    hs.mmtf_tuning(0)                                                        # (process-global)
    hs.rle8_mmtf_tuning(0)


def to_dev(data, offset=0):
    import torch

    t = torch.zeros(len(data) + offset + 64, dtype=torch.uint8, device="cuda")[offset : offset + len(data)]
    t.copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))
    return t


def compress_dev(hs, data, offsets=(0, 0, 0), extra=13, stream=None):
    """(size word, status word, the out buffer's bytes, nothing written outside [0, size)?).  Out buffer: 0xEE, workspace: 0xC3 garbage."""
    import torch

    n, cap = len(data), len(data) + extra
    src = to_dev(data, offsets[0])
    full = torch.full((offsets[1] + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dst = full[offsets[1] : offsets[1] + cap]
    ws = torch.full((hs.rle8_mmtf128_workspace_size(0, n) + offsets[2],), 0xC3, dtype=torch.uint8, device="cuda")[offsets[2] :]
    words = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    hs.rle8_mmtf128_compress_dev(src, dst, words[0:1], words[1:2], ws, stream=stream)
    torch.cuda.synchronize()
    size, status = (int(x) for x in words.cpu().numpy())
    host = full.cpu().numpy()
    clean = bool((host[: offsets[1]] == 0xEE).all() and (host[offsets[1] + size :] == 0xEE).all())
    return size, status, host[offsets[1] : offsets[1] + cap].tobytes(), clean


def decompress_dev(hs, stream, n, offsets=(0, 0, 0)):
    """(status word, output bytes, canary around the output intact?)"""
    import torch

    src = to_dev(stream, offsets[0])
    full = torch.full((offsets[1] + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dst = full[offsets[1] : offsets[1] + n]
    ws = torch.full((hs.rle8_mmtf128_workspace_size(1, n) + offsets[2],), 0xC3, dtype=torch.uint8, device="cuda")[offsets[2] :]
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hs.rle8_mmtf128_decompress_dev(src, dst, status, ws)
    torch.cuda.synchronize()
    host = full.cpu().numpy()
    clean = bool((host[: offsets[1]] == 0xEE).all() and (host[offsets[1] + n :] == 0xEE).all())
    return int(status.item()), host[offsets[1] : offsets[1] + n].tobytes(), clean


def check_both_ways(hs, name, data, offsets=(0, 0, 0)):
    want = model_stream(data)
    size, status, out, clean = compress_dev(hs, data, offsets)
    assert (status, size) == (DONE, len(want)), name
    assert out[:size] == want, f"{name}: the stream differs from the model's"
    assert clean, f"{name}: compress wrote outside [0, size)"
    status, back, clean = decompress_dev(hs, want, len(data), offsets)
    assert status == DONE, name
    assert back == data, f"{name}: decode differs"
    assert clean, f"{name}: decompress wrote outside [0, size)"


@pytest.mark.parametrize("name", list(CASES))
def test_every_packet_shape(hs, name):
    check_both_ways(hs, name, CASES[name])


@pytest.mark.parametrize("span", (1, 7, 63, 0))
@pytest.mark.parametrize("segment", (2, 7, 0))
def test_segment_and_span_lengths_give_the_same_bytes(tuned, segment, span):
    """mmtf segments of 2 and 7 rows put a segment edge inside every packet of more rows; spans of 1, 7, 63 rows move every span edge"""
    tuned.mmtf_tuning(segment)
    tuned.rle8_mmtf_tuning(span)
    for name in SMALL:
        check_both_ways(tuned, f"{name} segment {segment} span {span}", CASES[name])


@pytest.mark.parametrize("offsets", ((1, 3, 5), (3, 17, 1), (17, 1, 3)))
def test_odd_addresses(hs, offsets):
    for name in ("copy_31_32", "span_edge_3bit", "span_edge_2bit", "span_edge_4bit", "alphabet256_5000", "zeros_17"):
        check_both_ways(hs, name, CASES[name], offsets)


def test_reference_bound_is_short_for_incompressible_input(hs):
    """32 literal 8 bit rows and more need inSize + 13 bytes (include/hsrle.h): with the reference's bound as capacity the verdict is CAPACITY and
    nothing is written; with 13 the stream is the model's."""
    rows = T.literal_rows(64, 255, random.Random(3))
    data = T.data_from_rank_rows(rows)
    assert len(model_stream(data)) == len(data) + 13
    size, status, out, clean = compress_dev(hs, data, extra=8)
    assert (size, status) == (0, CAPACITY)
    assert clean and out == b"\xEE" * len(out)
    assert hs.rle8_mmtf128_compress(data, out_cap=len(data) + 8) == (0, b"")
    assert hs.rle8_mmtf128_compress(data) == (len(data) + 13, model_stream(data))


def golden():
    with open(T.GOLDEN) as f:
        return json.load(f)["vectors"]


def test_decode_of_the_references_stored_streams(hs):
    for v in golden():
        data, stream = bytes.fromhex(v["input"]), bytes.fromhex(v["stream"])
        status, back, clean = decompress_dev(hs, stream, len(data))
        assert (status, back, clean) == (DONE, data, True), v["name"]


def grammar_streams():
    """Legal streams no encoder writes."""
    rng = random.Random(21)
    end = ("rle", 0, None, False)
    out = {}
    for code in range(4):
        # a first COPY of no rows with each flag value; a null COPY in long form; the terminator in long form
        out[f"first_null_copy_code{code}"] = (48, [("copy", [], code, False), ("rle", 2, 5, False), ("copy", [], code, True), ("rle", 1, 5, False), ("copy", [], 0, False),
                                                   ("rle", 0, None, True)], b"")
        # 4-byte COPY headers with counts below 32, rows narrower than their width
        rows = T.literal_rows(7, 3, rng)
        out[f"long_copy_header_code{code}"] = (16 * 9 + 2, [("copy", rows, code, True), ("rle", 2, 0, True), ("copy", [], 0, False), end], b"\x07\x01")
        # a COPY packet that holds uniform rows, of every group remainder
        for k in (1, 4, 6, 13):
            rows = T.literal_rows(k, 3, rng) + [b"\x02" * 16]
            out[f"uniform_rows_in_copy_code{code}_{k + 1}"] = (16 * (k + 1), [("copy", rows, code, False), end], b"")
    # 4-byte RLE headers with counts below 128; RLE counts larger than rank + 1; null COPYs in front of an RLE that continues the same rank
    lit = T.literal_rows(3, 200, rng)
    out["long_rle_headers"] = (16 * 30 + 1, [("copy", lit, 0, False), ("rle", 10, 2, True), ("copy", [], 0, False), ("rle", 7, 2, False), ("copy", [], 6 >> 1, False),
                                             ("rle", 5, 1, True), ("copy", [], 0, True), ("rle", 5, 0, False), ("copy", [], 0, False), end], b"\x09")
    out["rle_counts_above_rank_plus_one"] = (16 * 300, [("copy", [], 3, False), ("rle", 100, 3, False), ("copy", [], 0, False), ("rle", 130, 1, True), ("copy", [], 0, False),
                                                        ("rle", 70, 200, False), ("copy", [], 0, False), end], b"")
    return {k: T.write_stream(n, packets, tail) for k, (n, packets, tail) in out.items()}


def test_decode_of_grammar_written_streams(hs):
    for name, stream in grammar_streams().items():
        want = T.model_decompress(stream)
        assert want is not None, name
        status, back, clean = decompress_dev(hs, stream, len(want))
        assert (status, clean) == (DONE, True), name
        assert back == want, name
        assert hs.rle8_mmtf128_decompress(stream, len(want) + 5) == (len(want), want), name


def malformed_streams():
    rng = random.Random(33)
    rows = T.literal_rows(6, 200, rng)
    end = ("rle", 0, None, False)
    good = T.write_stream(96, [("copy", rows, 0, False), end])
    out = {
        "body_past_stream_size": (96, T.write_stream(96, [("copy", rows, 0, False), end], stream_size=8 + 1 + 50)),
        "long_body_past_stream_size": (96, struct.pack("<III", 96, 8 + 4 + 96 + 1, 0x1FFFFFF << 3 | 1) + b"".join(rows) + b"\x00"),
        "copy_rows_past_R": (80, T.write_stream(80, [("copy", rows, 0, False), end])),
        "rle_rows_past_R": (96, T.write_stream(96, [("copy", rows[:3], 0, False), ("rle", 4, 1, False), ("copy", [], 0, False), end])),
        "huge_rle_count": (96, T.write_stream(96, [("copy", [], 0, False), ("rle", 0x7FFFFFFF, 1, True), ("copy", [], 0, False), end])),
        "missing_terminator": (96, T.write_stream(96, [("copy", rows, 0, False)])),
        "chain_goes_on_behind_the_rows": (96, T.write_stream(96, [("copy", rows, 0, False), ("rle", 1, 0, False), ("copy", [], 0, False), end])),
        "rows_left_over": (112, T.write_stream(112, [("copy", rows, 0, False), end])),
        "tail_past_stream_size": (99, T.write_stream(99, [("copy", rows, 0, False), end], b"\x01\x02")),
        "header_size_is_not_the_output_size": (80, good),
        "stream_size_above_the_buffer": (96, good[:4] + struct.pack("<I", len(good) + 1) + good[8:]),
    }
    return good, out


def test_malformed_streams_are_refused_before_any_write(hs):
    good, bad = malformed_streams()
    assert decompress_dev(hs, good, 96)[0] == DONE
    for name, (n, stream) in bad.items():
        if name not in ("header_size_is_not_the_output_size", "stream_size_above_the_buffer"):
            assert T.model_decompress(stream) is None, name
        status, _, clean = decompress_dev(hs, stream, n)
        assert status == MALFORMED, name
        assert clean, f"{name}: the canary around the output was touched"
        if name != "header_size_is_not_the_output_size":
            assert hs.rle8_mmtf128_decompress(stream, n + 64) == (0, b""), name


def test_drop_in_functions(hs):
    assert hs.rle8_mmtf128_compress_bounds(1000) == 1008 and hs.rle8_mmtf256_compress_bounds((1 << 30) + 1) == 0
    for name in ("zeros_1", "random_15", "zeros_16", "random_17", "copy_31_32", "rle_127_128", "span_edge_3bit", "every_symbol_per_column", "video_70000"):
        data = CASES[name]
        want = model_stream(data)
        assert hs.rle8_mmtf128_compress(data) == (len(want), want), name
        assert hs.rle8_mmtf128_decompress(want, len(data)) == (len(data), data), name
        assert hs.rle8_mmtf128_decompress(want + bytes(7), len(data) + 9) == (len(data), data), name
        assert hs.rle8_mmtf128_decompress(want, len(data) - 1)[0] == 0, name                # header inSize > outSize
        assert hs.rle8_mmtf128_decompress(want[:-1], len(data))[0] == 0, name               # header streamSize > inSize
    assert hs.rle8_mmtf128_compress(b"")[0] == 0
    assert hs.rle8_mmtf128_compress(bytes(32), out_cap=39)[0] == 0


def test_graph_capture_and_replay(hs):
    """Compress and decompress captured once on a side stream and replayed on new bytes, the workspaces refilled with garbage before each replay.
    (The decode's stream length is part of the captured call: the replays' inputs are chosen to give streams of the same size.)"""
    import torch

    n = 16 * 200 + 5
    specs = [[("copy", 40, 3), ("rle", 100, 0), ("copy", 60, 200)], [("copy", 40, 3), ("rle", 100, 7), ("copy", 60, 255)], [("copy", 40, 2), ("rle", 100, 255), ("copy", 60, 128)]]
    inputs = [from_spec(s, b"\x01\x02\x03\x04\x05", seed=i) for i, s in enumerate(specs)]
    sizes = {len(model_stream(d)) for d in inputs}
    assert len(sizes) == 1
    size = sizes.pop()
    src = to_dev(inputs[0])
    enc = torch.full((n + 13 + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dec = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    ws1 = torch.full((hs.rle8_mmtf128_workspace_size(0, n),), 0xC3, dtype=torch.uint8, device="cuda")
    ws2 = torch.full((hs.rle8_mmtf128_workspace_size(1, n),), 0xC3, dtype=torch.uint8, device="cuda")
    words = torch.full((3,), -1, dtype=torch.int32, device="cuda")

    def both(stream):
        hs.rle8_mmtf128_compress_dev(src, enc[: n + 13], words[0:1], words[1:2], ws1, stream=stream)
        hs.rle8_mmtf128_decompress_dev(enc[:size], dec[:n], words[2:3], ws2, stream=stream)

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        both(side)                                                           # warm-up outside the capture (module load)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        both(side)
    for data in inputs[1:]:
        src.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
        enc.fill_(0xEE)
        dec.fill_(0xEE)
        ws1.fill_(0x5A)
        ws2.fill_(0xA5)
        words.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        e, d = enc.cpu().numpy(), dec.cpu().numpy()
        assert [int(x) for x in words.cpu().numpy()] == [size, DONE, DONE]
        assert e[:size].tobytes() == model_stream(data)
        assert d[:n].tobytes() == data
        assert (e[size:] == 0xEE).all() and (d[n:] == 0xEE).all()
