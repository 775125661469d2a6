"""The checkpoints and the byte-range decode of rle8_mmtf128 streams as a model, without a GPU (tests/rle8_mmtf_range_testlib.py).  The checkpoint lists
are pinned to the transform: encoding the rest of the input from checkpoint k's lists gives the ranks that the encode of the whole input has from row
k * checkpointRows on -- the sequential definition's (mmtf_testlib) always, the compiled reference's where it is built.  The range decode, done the way the
device does it, gives data[offset : offset + length] over every stream of the index's cases, and refuses sidecars that do not go with the stream."""
import struct

import pytest

import mmtf_testlib as mt
import rle8_mmtf_index_testlib as X
import rle8_mmtf_range_testlib as G
import rle8_mmtf_testlib as T


def transform_inputs():
    out = {}
    for rows in (130, 257, 600):
        n = 16 * rows + rows % 16
        out[f"random_256_{rows}"] = mt.random_bytes(n, 256, 5)
        out[f"random_5_{rows}"] = mt.random_bytes(n, 5, 6)
        out[f"every_symbol_per_column_{rows}"] = mt.every_symbol_per_column(n, 16)
        out[f"late_symbols_in_some_columns_{rows}"] = mt.late_symbols_in_some_columns(n, 16, 64)
        out[f"video_shaped_{rows}"] = mt.video_shaped(n)
    return out


TRANSFORM_INPUTS = transform_inputs()
STREAMS = G.range_streams()


def encode_from(lists, data):
    """mmtf128 ranks of whole rows `data`, the sixteen lists started as given"""
    lists = [list(l) for l in lists]
    out = bytearray()
    for i, x in enumerate(data):
        l = lists[i % 16]
        k = l.index(x)
        out.append(k)
        if k:
            l.insert(0, l.pop(k))
    return bytes(out)


def check_lists_continue(encode_whole):
    for name, data in TRANSFORM_INPUTS.items():
        ranks = encode_whole(data)
        rows = len(data) // 16
        for ck_rows in G.CHECKPOINT_ROWS:
            in_size, _, got_rows, checkpoints = G.unpack_checkpoints(G.model_checkpoints(data, ck_rows, stream_size=10))
            assert (in_size, got_rows, len(checkpoints)) == (len(data), ck_rows, (rows - 1) // ck_rows), name
            for k, lists in enumerate(checkpoints, 1):
                assert all(sorted(l) == list(range(256)) for l in lists), name
                lo = 16 * k * ck_rows
                assert encode_from(lists, data[lo : 16 * rows]) == ranks[lo : 16 * rows], f"{name}: checkpoint {k} of {ck_rows} rows"


def test_checkpoint_lists_continue_the_sequential_encode():
    check_lists_continue(lambda data: mt.mmtf_enc(data, 16))


def test_checkpoint_lists_continue_the_references_encode():
    if not mt.MmtfReference.available():
        pytest.skip("oracle/_ref/libhsrle_ref.so not built (needs the reference's sources)")
    ref = mt.MmtfReference()

    def whole(data):
        rc, out = ref.run(mt.MMTF128, 0, data)
        assert rc == len(data)
        return out

    check_lists_continue(whole)


def test_sidecar_layout_and_counts():
    data = TRANSFORM_INPUTS["random_5_257"]
    side = G.model_checkpoints(data, 64, stream_size=1234)
    assert side[:8] == b"HSRLEMFC" and struct.unpack_from("<IIIIIIQ", side, 8) == (1, 64, len(data), 1234, 64, 4, 64 + 4 * 4096) and side[40:64] == bytes(24)
    assert len(side) == 64 + 4 * 4096
    for rows, ck_rows, count in ((0, 64, 0), (1, 64, 0), (64, 64, 0), (65, 64, 1), (128, 64, 1), (129, 64, 2), (129, 128, 1)):
        assert G.checkpoint_count(16 * rows + 3, ck_rows) == count
    assert G.model_checkpoints(data[: 16 * 64], 64, 10)[64:] == b"" and G.model_checkpoints(data[:13], 64, 10)[64:] == b""
    # a function of the data alone: what the stream looks like does not matter
    assert G.model_checkpoints(data, 128, 10)[64:] == G.model_checkpoints(data, 128, 99)[64:]


@pytest.mark.parametrize("ck_rows", G.CHECKPOINT_ROWS)
def test_range_decode_gives_the_inputs_bytes(ck_rows):
    for name, (stream, data) in STREAMS.items():
        index = X.model_index(stream, 64)
        side = G.model_checkpoints(data, ck_rows, len(stream))
        for offset, length in G.range_grid(len(data)):
            assert G.model_range_decode(stream, index, side, offset, length) == data[offset : offset + length], f"{name} [{offset}, +{length})"


def test_the_grid_holds_the_cases_it_is_for():
    """ranges that end in the tail, inside one long RLE, inside a COPY body above the walk's 1 KiB window, and the stream of under one row"""
    data = STREAMS["long_rle"][1]
    n = len(data)
    grid = G.range_grid(n)
    assert n % 16 == 15 and (n - 1, 1) in grid and (n - 17, 17) in grid and (0, n) in grid
    assert (16 * 64, 1024) in grid                                       # rows 64 .. 127 of the RLE of rows 5 .. 304
    data = STREAMS["long_8bit_copy"][1]
    assert (16 * 64 + 1, 1024) in G.range_grid(len(data))                # inside the 8 bit COPY of rows 60 .. 134: 1200 body bytes
    data = STREAMS["under_one_row"][1]
    assert len(data) == 13 and (1, 12) in G.range_grid(13) and G.range_rows(13, 1, 12, 64) == (0, 0)
    # a range of tail bytes alone behind a last row that is a checkpoint row's neighbour: through the last row, from the checkpoint in front of it
    assert G.range_rows(16 * 128 + 3, 16 * 128 + 1, 2, 64) == (64, 128) and G.range_rows(16 * 129 + 3, 16 * 129 + 1, 2, 64) == (128, 129)
    assert G.range_rows(16 * 300, 16 * 64 - 1, 2, 64) == (0, 65) and G.range_rows(16 * 300, 16 * 64, 16, 64) == (64, 65)


def test_sidecars_that_do_not_go_with_the_stream_are_refused():
    a, b = X.tamper_base()
    data = T.model_decompress(a)
    index, side = X.model_index(a, 64), G.model_checkpoints(data, 64, len(a))
    rows = len(data) // 16
    offset, length = 16 * 130 + 5, 16 * 100
    want = data[offset : offset + length]
    assert G.model_range_decode(a, index, side, offset, length) == want
    used = 64 + 4096 * (130 // 64 - 1)
    dup = side[:used + 256 * 3] + bytes([side[used + 256 * 3 + 1]]) + side[used + 256 * 3 + 1 :]          # column 3: rank 0's symbol twice
    with pytest.raises(G.CheckpointMismatch):
        G.model_range_decode(a, index, dup, offset, length)
    other = 64 + 4096 * (rows // 64 - 2)
    assert other != used
    dup = side[:other] + bytes([side[other + 1]]) + side[other + 1 :]
    assert G.model_range_decode(a, index, dup, offset, length) == want                                       # a checkpoint the range does not use
    for at in (8, 16, 20, 24, 28, 32, 63):
        with pytest.raises(G.CheckpointMismatch):
            G.model_range_decode(a, index, side[:at] + bytes([side[at] ^ 1]) + side[at + 1 :], offset, length)
    # index tampers inside the range's stretches
    entries = X.unpack_index(index)[3]
    inside = [k for k, e in enumerate(entries) if 128 <= e[1] < 231]
    assert len(inside) >= 2
    for name, bad in X.single_field_tampers(index).items():
        if any(name.startswith(f"entry{k}_") for k in inside):
            with pytest.raises(X.IndexMismatch):
                G.model_range_decode(a, bad, side, offset, length)
                pytest.fail(f"{name} was accepted")
    with pytest.raises(X.IndexMismatch):
        G.model_range_decode(a, X.model_index(b, 64), side, offset, length)
    with pytest.raises(T.Malformed):
        G.model_range_decode(a[:4] + struct.pack("<I", len(a) + 1) + a[8:], index, side, offset, length)
