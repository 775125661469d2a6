"""The entry index of rle8_mmtf128 streams on the GPU (csrc/hsrle_rle8mmtf_index.hip.h) against its model (tests/rle8_mmtf_index_testlib.py, held against
the serial parse by test_rle8_mmtf_index_model.py).  The encoder's index, the serial build's index and the model's are the same bytes; the stream of
compress_indexed is the plain compress's; the indexed decode gives the input with DONE and writes nothing outside its output.  An index that does not
agree with its stream -- any field of any entry, the order, the count, another stream's index -- ends in INDEX, never in wrong bytes marked DONE."""
import json

import numpy as np
import pytest

import rle8_mmtf_index_testlib as X
import rle8_mmtf_testlib as T

pytestmark = pytest.mark.gpu

GUARD = 4096
DONE, MALFORMED, CAPACITY, INDEX = 0, 1, 2, 3
INPUTS = X.encoder_inputs()
GRAMMAR = {**X.grammar_index_streams(), **X.restated_grammar_streams()}
_MODEL = {}


def model_stream(data):
    if data not in _MODEL:
        _MODEL[data] = T.model_compress(data)
    return _MODEL[data]


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


def to_dev(data, offset=0, slack=64):
    import torch

    t = torch.zeros(len(data) + offset + slack, dtype=torch.uint8, device="cuda")[offset : offset + len(data)]
    t.copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))
    return t


def guarded(n, offset):
    """(whole buffer of 0xEE, the n bytes at `offset` of it)"""
    import torch

    full = torch.full((offset + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    return full, full[offset : offset + n]


def untouched(full, offset, n):
    host = full.cpu().numpy()
    return bool((host[:offset] == 0xEE).all() and (host[offset + n :] == 0xEE).all())


def workspace(hs, decode, n, offset):
    import torch

    return torch.full((hs.rle8_mmtf128_workspace_size(decode, n) + offset,), 0xC3, dtype=torch.uint8, device="cuda")[offset:]


def compress_indexed_dev(hs, data, spacing=64, offsets=(0, 0, 0, 0), extra=13, index_cap=None):
    """(stream size, status, stream bytes, index size, index bytes, nothing written outside the stream and the index?); offsets: input, output, workspace, index"""
    import torch

    n, cap = len(data), len(data) + extra
    icap = hs.rle8_mmtf128_index_bound(n, spacing) if index_cap is None else index_cap
    src = to_dev(data, offsets[0])
    full, dst = guarded(cap, offsets[1])
    ifull, idx = guarded(icap, offsets[3])
    words = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    isize = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    hs.rle8_mmtf128_compress_indexed_dev(src, dst, words[0:1], words[1:2], workspace(hs, 0, n, offsets[2]), idx, isize, spacing_rows=spacing)
    torch.cuda.synchronize()
    size, status = (int(x) for x in words.cpu().numpy())
    isz = int(isize.item())
    clean = untouched(full, offsets[1], size) and untouched(ifull, offsets[3], isz)
    return size, status, dst.cpu().numpy().tobytes()[:size], isz, idx.cpu().numpy().tobytes()[:isz], clean


def index_build_dev(hs, stream, n, spacing=64, offsets=(0, 0)):
    """(status, index size, index bytes, the whole index buffer's bytes, nothing written outside the index?); offsets: stream, index"""
    import torch

    icap = hs.rle8_mmtf128_index_bound(n, spacing)
    src = to_dev(stream, offsets[0])
    ifull, idx = guarded(icap, offsets[1])
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    isize = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    hs.rle8_mmtf128_index_build_dev(src, n, idx, isize, status, spacing_rows=spacing)
    torch.cuda.synchronize()
    isz = int(isize.item())
    whole = idx.cpu().numpy().tobytes()
    return int(status.item()), isz, whole[:isz], whole, untouched(ifull, offsets[1], icap)


def info_of(hs, index):
    return hs.rle8_mmtf128_index_info(index)


def decompress_indexed_dev(hs, stream, index, n, offsets=(0, 0, 0, 0), info=None):
    """(status, output bytes, canary around the output intact?); offsets: stream, output, workspace, index.  The index buffer has 64 bytes of slack."""
    import torch

    src = to_dev(stream, offsets[0])
    idx = to_dev(index, offsets[3])
    full, dst = guarded(n, offsets[1])
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hs.rle8_mmtf128_decompress_indexed_dev(src, idx, info_of(hs, index) if info is None else info, dst, status, workspace(hs, 1, n, offsets[2]))
    torch.cuda.synchronize()
    return int(status.item()), dst.cpu().numpy().tobytes(), untouched(full, offsets[1], n)


def check_input(hs, name, data, spacing=64, offsets=(0, 0, 0, 0)):
    stream = model_stream(data)
    want = X.model_index(stream, spacing)
    size, status, got, isz, index, clean = compress_indexed_dev(hs, data, spacing, offsets)
    assert (status, size) == (DONE, len(stream)), name
    assert got == stream, f"{name}: the stream differs from the plain compress's"
    assert (isz, index) == (len(want), want), f"{name}: the encoder's index differs from the model's"
    assert clean, f"{name}: compress_indexed wrote outside the stream or the index"
    check_stream(hs, name, stream, data, spacing, offsets)


def check_stream(hs, name, stream, data, spacing=64, offsets=(0, 0, 0, 0)):
    want = X.model_index(stream, spacing)
    status, isz, index, _, clean = index_build_dev(hs, stream, len(data), spacing, (offsets[0], offsets[3]))
    assert (status, isz, index, clean) == (DONE, len(want), want, True), f"{name}: the built index differs from the model's"
    status, back, clean = decompress_indexed_dev(hs, stream, want, len(data), offsets)
    assert status == DONE, name
    assert back == data, f"{name}: the indexed decode differs"
    assert clean, f"{name}: the indexed decode wrote outside its output"


def test_every_case(hs):
    for name, data in INPUTS.items():
        size, status, plain, _ = plain_compress(hs, data)
        assert (status, plain) == (DONE, model_stream(data)), name
        check_input(hs, name, data)


def plain_compress(hs, data):
    import torch

    n = len(data)
    full, dst = guarded(n + 13, 0)
    words = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    hs.rle8_mmtf128_compress_dev(to_dev(data), dst, words[0:1], words[1:2], workspace(hs, 0, n, 0))
    torch.cuda.synchronize()
    size, status = (int(x) for x in words.cpu().numpy())
    return size, status, dst.cpu().numpy().tobytes()[:size], untouched(full, 0, size)


def test_grammar_written_streams(hs):
    for name, stream in GRAMMAR.items():
        data = T.model_decompress(stream)
        assert data is not None, name
        check_stream(hs, name, stream, data)


def test_other_spacings(hs):
    """128 and 1024 rows; 0 is the library's default: the header says which"""
    a, b = X.tamper_base()
    big = T.data_from_rank_rows(T.rows_from_spec([("copy", 700, 3), ("rle", 900, 1), ("copy", 40, 255), ("rle", 600, 0), ("copy", 1100, 15)], seed=4), b"\x01\x02")
    for name, data in (("tamper_base", T.model_decompress(a)), ("alternating_one_row_packets", INPUTS["alternating_one_row_packets"]), ("big", big)):
        for spacing in (128, 1024):
            check_input(hs, f"{name} spacing {spacing}", data, spacing)
        size, status, got, isz, index, clean = compress_indexed_dev(hs, data, 0)
        assert (status, got, clean) == (DONE, model_stream(data), True), name
        rows = info_of(hs, index).spacing
        assert rows in (256, 1024, 4096) and index == X.model_index(got, rows), name
        assert index_build_dev(hs, got, len(data), 0)[2] == index, name
        assert decompress_indexed_dev(hs, got, index, len(data))[:2] == (DONE, data), name


def test_odd_addresses(hs):
    for offsets in ((1, 3, 5, 7), (3, 17, 1, 9), (17, 1, 3, 2)):
        for name in ("entry_on_rle_behind_rle", "long_8bit_copy", "alternating_one_row_packets", "long_rle", "under_one_row"):
            check_input(hs, f"{name} at {offsets}", INPUTS[name], 64, offsets)
        for name in ("null_copy_long_in_front_of_entry", "long_headers_on_entries", "ends_rle_long_nullcopy_long_rle0_tail15"):
            check_stream(hs, f"{name} at {offsets}", GRAMMAR[name], T.model_decompress(GRAMMAR[name]), 64, offsets)


def test_segment_and_span_lengths_give_the_same_bytes(tuned):
    """spans of 1, 7 and 63 rows move every span edge off the window edges: the index is the same; mmtf segments of 2 and 7 rows as the codec's own test has them"""
    a, _ = X.tamper_base()
    for segment in (2, 7, 0):
        for span in (1, 7, 63):
            tuned.mmtf_tuning(segment)
            tuned.rle8_mmtf_tuning(span)
            for name, data in INPUTS.items():
                check_input(tuned, f"{name} segment {segment} span {span}", data)
            check_input(tuned, f"tamper_base segment {segment} span {span} spacing 128", T.model_decompress(a), 128)


def test_the_references_stored_streams(hs):
    with open(T.GOLDEN) as f:
        vectors = json.load(f)["vectors"]
    for v in vectors:
        data, stream = bytes.fromhex(v["input"]), bytes.fromhex(v["stream"])
        check_stream(hs, v["name"], stream, data)


def test_capacity_leaves_no_index(hs):
    """the stream does not fit: size words 0, nothing written, no magic"""
    import random

    data = T.data_from_rank_rows(T.literal_rows(80, 255, random.Random(3)))
    size, status, _, isz, _, clean = compress_indexed_dev(hs, data, extra=8)
    assert (size, status, isz, clean) == (0, CAPACITY, 0, True)


@pytest.fixture(scope="module")
def base(hs):
    a, b = X.tamper_base()
    data = T.model_decompress(a)
    index = X.model_index(a, 64)
    assert decompress_indexed_dev(hs, a, index, len(data)) == (DONE, data, True)
    return a, b, data, index


def test_single_field_tampers_end_in_index(hs, base):
    a, _, data, index = base
    for name, bad in X.single_field_tampers(index).items():
        status, _, clean = decompress_indexed_dev(hs, a, bad, len(data))
        assert (status, clean) == (INDEX, True), name


def test_structural_tampers_end_in_index(hs, base):
    a, b, data, index = base
    tampers = X.structural_tampers(a, index)
    tampers["the_index_of_another_stream"] = X.model_index(b, 64)
    for name, bad in tampers.items():
        info = None
        if name in ("count_plus_one", "count_minus_one"):                # the count field alone, `info` patched to match
            info = info_of(hs, index)
            info.recordCount += 1 if name == "count_plus_one" else -1
        status, _, clean = decompress_indexed_dev(hs, a, bad, len(data), info=info)
        assert (status, clean) == (INDEX, True), name
    # an index header on the device that differs from `info`: every field of it
    for field, value in (("compressedSize", len(a) - 1), ("recordCount", 4)):
        info = info_of(hs, index)
        setattr(info, field, value)
        status, _, clean = decompress_indexed_dev(hs, a, index, len(data), info=info)
        assert (status, clean) == (INDEX, True), field
    wider = X.model_index(a, 128)                                        # (fewer entries: a count that spacing 64 may hold too)
    info = info_of(hs, wider)
    info.spacing = 64
    status, _, clean = decompress_indexed_dev(hs, a, wider, len(data), info=info)
    assert (status, clean) == (INDEX, True), "spacing"
    for at in (0, 8, 12, 40, 63):
        bad = index[:at] + bytes([index[at] ^ 1]) + index[at + 1 :]
        status, _, clean = decompress_indexed_dev(hs, a, bad, len(data), info=info_of(hs, index))
        assert (status, clean) == (INDEX, True), at


def test_true_headers_that_are_not_the_rules_choice_are_accepted(hs, base):
    a, _, data, index = base
    in_size, stream_size, spacing, entries = X.unpack_index(index)
    for name, chosen in (("one_left_out", entries[:1] + entries[2:]), ("none", []), ("every_packet_with_rows", [(p, r, n, k) for p, r, n, k, c in X.header_positions(a) if c and r][:5])):
        other = X.pack_index(in_size, stream_size, spacing, chosen)
        assert decompress_indexed_dev(hs, a, other, len(data)) == (DONE, data, True), name


def test_stream_header_against_the_arguments_stays_malformed(hs, base):
    a, _, data, index = base
    bad = a[:4] + (len(a) + 1).to_bytes(4, "little") + a[8:]                 # streamSize above the buffer
    status, _, clean = decompress_indexed_dev(hs, bad, index, len(data))
    assert (status, clean) == (MALFORMED, True)
    bad = (len(data) - 16).to_bytes(4, "little") + a[4:]                     # header inSize is not the output size
    status, _, clean = decompress_indexed_dev(hs, bad, index, len(data))
    assert (status, clean) == (MALFORMED, True)


def test_a_stream_corrupted_in_a_middle_stretch(hs, base):
    a, _, data, index = base
    entries = X.unpack_index(index)[3]
    for name, at, flip in (("count_of_an_entrys_packet", entries[2][0], 0x10), ("count_inside_a_stretch", entries[1][0], 0x08), ("rank_of_an_rle", entries[0][0] + 1, 0x01)):
        bad = a[:at] + bytes([a[at] ^ flip]) + a[at + 1 :]
        status, back, clean = decompress_indexed_dev(hs, bad, index, len(data))
        assert clean, name
        if name == "rank_of_an_rle":                                     # no header changes: a good stream of other bytes, as the plain decode says too
            assert (status, back) == (DONE, T.model_decompress(bad)) and back != data, name
        else:
            assert status != DONE, name


def test_malformed_streams_through_index_build(hs):
    for name, (n, stream) in X.malformed_streams().items():
        status, isz, _, whole, clean = index_build_dev(hs, stream, n)
        assert (status, isz, clean) == (MALFORMED, 0, True), name
        assert X.MAGIC not in whole, f"{name}: the magic was written"


def test_graph_capture_and_replay(hs, base):
    """The indexed decode captured once and replayed on a second stream and index in the same buffers (same sizes, same entry count), the workspace
    refilled with garbage; then on the first stream with the second's index: INDEX."""
    import torch

    a, b, data_a, index_a = base
    data_b, index_b = T.model_decompress(b), X.model_index(b, 64)
    assert len(a) == len(b) and len(index_a) == len(index_b) and len(data_a) == len(data_b)
    n = len(data_a)
    src, idx = to_dev(a), to_dev(index_a)
    full, dst = guarded(n, 0)
    ws = workspace(hs, 1, n, 0)
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    info = info_of(hs, index_a)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        hs.rle8_mmtf128_decompress_indexed_dev(src, idx, info, dst, status, ws, stream=side)    # warm-up outside the capture (module load)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        hs.rle8_mmtf128_decompress_indexed_dev(src, idx, info, dst, status, ws, stream=side)
    for stream, index, want_status, want in ((b, index_b, DONE, data_b), (a, index_a, DONE, data_a), (a, index_b, INDEX, None), (b, index_b, DONE, data_b)):
        src.copy_(torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()))
        idx.copy_(torch.from_numpy(np.frombuffer(index, dtype=np.uint8).copy()))
        full.fill_(0xEE)
        ws.fill_(0x5A)
        status.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert int(status.item()) == want_status
        assert untouched(full, 0, n)
        if want is not None:
            assert dst.cpu().numpy().tobytes() == want


def test_host_calls(hs, base):
    a, b, data, index = base
    for name, stream, want in [("tamper_base", a, data)] + [(k, model_stream(v), v) for k, v in INPUTS.items() if k in ("no_entry", "long_rle", "under_one_row")]:
        rc, built = hs.rle8_mmtf128_index_build_host(stream, 64)
        assert (rc, built) == (hs.OK, X.model_index(stream, 64)), name
        assert hs.rle8_mmtf128_decompress_indexed_host(stream + bytes(5), built, len(want) + 3) == (hs.OK, want), name
    assert hs.rle8_mmtf128_decompress_indexed_host(a, X.model_index(b, 64), len(data)) == (hs.ERR_FORMAT, b"")
    assert hs.rle8_mmtf128_decompress_indexed_host(a, index, len(data) - 1) == (hs.ERR_CAPACITY, b"")
    n, bad = X.malformed_streams()["rows_left_over"]
    assert hs.rle8_mmtf128_index_build_host(bad, 64) == (hs.ERR_FORMAT, b"")
