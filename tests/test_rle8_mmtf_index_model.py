"""The entry index of rle8_mmtf128 streams as a model, without a GPU (tests/rle8_mmtf_index_testlib.py): over the reference's stored streams, the
grammar-written streams and the index's own cases, at spacings 64, 128 and 1024 rows, the indexed parse gives the serial parse's packet list, every
entry is a header position of the serial parse, and every single-field tamper of an entry is refused."""
import json

import pytest

import rle8_mmtf_index_testlib as X
import rle8_mmtf_testlib as T


def streams():
    out = {}
    with open(T.GOLDEN) as f:
        for v in json.load(f)["vectors"]:
            out["golden_" + v["name"]] = bytes.fromhex(v["stream"])
    out.update(X.restated_grammar_streams())
    out.update(X.grammar_index_streams())
    for name, data in X.encoder_inputs().items():
        out[name] = T.model_compress(data)
    a, b = X.tamper_base()
    out["tamper_base_a"], out["tamper_base_b"] = a, b
    return out


STREAMS = streams()


@pytest.mark.parametrize("spacing", X.SPACINGS)
def test_indexed_parse_is_the_serial_parse(spacing):
    for name, stream in STREAMS.items():
        _, want, _ = T.parse_stream(stream)
        assert X.model_indexed_parse(stream, X.model_index(stream, spacing)) == want, name


@pytest.mark.parametrize("spacing", X.SPACINGS)
def test_entries_follow_the_rule(spacing):
    """every entry is a header of the serial parse, of a packet with rows, the first one that begins in its window; no window with such a packet is left out"""
    for name, stream in STREAMS.items():
        in_size, stream_size, sp, entries = X.unpack_index(X.model_index(stream, spacing))
        heads = X.header_positions(stream)
        assert (in_size, stream_size, sp) == (int.from_bytes(stream[:4], "little"), int.from_bytes(stream[4:8], "little"), spacing), name
        with_rows = [(pos, row, n, kind) for pos, row, n, kind, c in heads if c]
        assert [n for _, _, n, _ in with_rows] == list(range(len(with_rows))), name
        windows = {}
        for h in with_rows:
            windows.setdefault(h[1] // spacing, h)
        windows.pop(0, None)
        assert entries == [windows[j] for j in sorted(windows)], name
        assert len(X.model_index(stream, spacing)) <= 64 + 16 * max(0, (in_size // 16 - 1) // spacing if in_size >= 16 else 0), name


def test_the_cases_put_entries_where_they_say():
    """what the GPU test's case names promise, at spacing 64"""
    kinds = lambda name: [e[3] for e in X.unpack_index(X.model_index(STREAMS[name], 64))[3]]
    rows = lambda name: [e[1] for e in X.unpack_index(X.model_index(STREAMS[name], 64))[3]]
    assert kinds("no_entry") == [] and kinds("under_one_row") == []
    assert kinds("entry_on_copy") == [X.COPY] and rows("entry_on_copy") == [70]
    assert kinds("entry_on_rle_behind_copy")[0] == X.RLE and kinds("entry_on_rle_behind_rle")[:2] == [X.RLE, X.RLE]
    assert rows("begins_on_window_edge") == [64, 128, 192] and rows("begins_on_window_last_row") == [127, 191, 255]
    assert rows("long_8bit_copy") == [135, 205] and rows("long_rle") == [305, 345]         # windows without an entry
    assert rows("alternating_one_row_packets") == [64, 128, 192]
    for name, null_copy in (("null_copy_short_in_front_of_entry", b"\x00"), ("null_copy_long_in_front_of_entry", b"\x05\x00\x00\x00")):
        (off, row, n, kind), = X.unpack_index(X.model_index(STREAMS[name], 64))[3]
        assert (row, n, kind) == (70, 1, X.RLE) and STREAMS[name][off - len(null_copy) : off] == null_copy, name
    a, b = X.tamper_base()
    ia, ib = X.unpack_index(X.model_index(a, 64)), X.unpack_index(X.model_index(b, 64))
    assert ia[:3] == ib[:3] and len(ia[3]) == len(ib[3]) >= 5 and ia[3] != ib[3] and {e[3] for e in ia[3]} == {X.COPY, X.RLE}


def test_single_field_tampers_are_refused():
    a, _ = X.tamper_base()
    for spacing in X.SPACINGS:
        index = X.model_index(a, spacing)
        for name, bad in X.single_field_tampers(index).items():
            with pytest.raises(X.IndexMismatch):
                X.model_indexed_parse(a, bad)
                pytest.fail(f"spacing {spacing}: {name} was accepted")
    for name, stream in STREAMS.items():
        for tname, bad in X.single_field_tampers(X.model_index(stream, 64)).items():
            with pytest.raises(X.IndexMismatch):
                X.model_indexed_parse(stream, bad)
                pytest.fail(f"{name}: {tname} was accepted")


def test_structural_tampers_and_foreign_indexes():
    a, b = X.tamper_base()
    index = X.model_index(a, 64)
    for name, bad in X.structural_tampers(a, index).items():
        with pytest.raises(X.IndexMismatch):
            X.model_indexed_parse(a, bad)
            pytest.fail(f"{name} was accepted")
    with pytest.raises(X.IndexMismatch):
        X.model_indexed_parse(a, X.model_index(b, 64))
    # true packet headers in order that are not the rule's choice are accepted: the parse proves entries, not the rule
    in_size, stream_size, spacing, entries = X.unpack_index(index)
    _, want, _ = T.parse_stream(a)
    assert X.model_indexed_parse(a, X.pack_index(in_size, stream_size, spacing, entries[:1] + entries[2:])) == want
    heads = [(pos, row, n, kind) for pos, row, n, kind, c in X.header_positions(a) if c and row]
    assert X.model_indexed_parse(a, X.pack_index(in_size, stream_size, spacing, heads)) == want


def test_a_corrupted_stretch_is_refused():
    a, _ = X.tamper_base()
    index = X.model_index(a, 64)
    entries = X.unpack_index(index)[3]
    at = entries[2][0]                                                    # the header byte of a middle entry's packet
    bad = a[:at] + bytes([a[at] ^ 0x10]) + a[at + 1 :]                    # another count
    assert X.model_indexed_parse(a, index) == T.parse_stream(a)[1]
    with pytest.raises(X.IndexMismatch):
        X.model_indexed_parse(bad, index)
