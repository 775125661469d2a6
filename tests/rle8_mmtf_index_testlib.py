"""Helpers of the tests of the rle8_mmtf128 entry index (include/hsrle.h section 5; csrc/hsrle_rle8mmtf_index.hip.h): the index by THE RULE from the
serial parse of rle8_mmtf_testlib, the indexed parse -- the stretch walks with their entry checks and landing checks, as the device does them -- and the
streams and tampers both the model test and the GPU test run over.

Index: 64 header bytes ("HSRLEMFI", u32 version 1, u32 headerBytes 64, u32 uncompressedSize, u32 streamSize, u32 spacingRows, u32 entryCount,
u64 indexSize, zeros), then entryCount entries (u32 offset, u32 row, u32 ordinal, u32 kind: 0 COPY, 1 RLE).
"""
import random
import struct

import rle8_mmtf_testlib as T

MAGIC = b"HSRLEMFI"
HEADER = 64
COPY, RLE = 0, 1
SPACINGS = (64, 128, 1024)


class IndexMismatch(Exception):
    pass


def packet_bytes(p):
    """header and body bytes of a packet of parse_stream's list"""
    if p[0] == "copy":
        return (4 if p[3] else 1) + len(p[1]) * T.ROW_BYTES[p[2]]
    return (4 if p[3] else 1) + (1 if p[1] else 0)


def packet_rows(p):
    return len(p[1]) if p[0] == "copy" else p[1]


def header_positions(stream):
    """(offset, row, ordinal, kind, rows) of every packet of the serial parse, the null packets included"""
    _, packets, _ = T.parse_stream(stream)
    out, pos, row, n = [], 8, 0, 0
    for p in packets:
        c = packet_rows(p)
        out.append((pos, row, n, COPY if p[0] == "copy" else RLE, c))
        pos += packet_bytes(p)
        row += c
        n += 1 if c else 0
    return out


def pack_index(in_size, stream_size, spacing, entries):
    head = MAGIC + struct.pack("<IIIIIIQ", 1, HEADER, in_size, stream_size, spacing, len(entries), HEADER + 16 * len(entries))
    return head + bytes(HEADER - len(head)) + b"".join(struct.pack("<IIII", *e) for e in entries)


def unpack_index(index):
    """(in_size, stream_size, spacing, [entries as tuples]) of index bytes whose header is taken on trust"""
    version, header, in_size, stream_size, spacing, count, size = struct.unpack_from("<IIIIIIQ", index, 8)
    assert index[:8] == MAGIC and (version, header, size) == (1, HEADER, HEADER + 16 * count) and len(index) >= size
    return in_size, stream_size, spacing, [struct.unpack_from("<IIII", index, HEADER + 16 * k) for k in range(count)]


def model_index(stream, spacing):
    """The index by the rule: per window j >= 1 of `spacing` rows the first non-null packet whose first row lies in it."""
    in_size, stream_size = struct.unpack_from("<II", stream, 0)
    entries, seen = [], 0
    for pos, row, n, kind, c in header_positions(stream):
        if c and row // spacing > seen:
            seen = row // spacing
            entries.append((pos, row, n, kind))
    return pack_index(in_size, stream_size, spacing, entries)


def _walk(stream, S, R, tail, pos, row, n, rle, end, max_rec):
    """One stretch, as d_rm_walk_from does it: the packets (in parse_stream's form) from (pos, row, n) up to `end` (offset, row, ordinal, kind), or to the
    chain's end without one.  Raises IndexMismatch for a packet the serial walk refuses, a missed or passed landing, a chain that ends early."""
    packets = []
    row_end, rec_end = (end[1], end[2]) if end else (R, max_rec)

    def landed(kind):
        if end is None:
            return False
        if pos == end[0]:
            if (row, n, kind) != end[1:]:
                raise IndexMismatch("stands on the entry in another state")
            return True
        if pos > end[0] or row > end[1]:
            raise IndexMismatch("passed the entry")
        return False

    while True:
        if not rle:
            if landed(COPY):
                return packets, pos, row, n
            if pos >= S:
                raise IndexMismatch("COPY header")
            b = stream[pos]
            h = 4 if b & 1 else 1
            if pos + h > S:
                raise IndexMismatch("COPY header")
            c = (struct.unpack_from("<I", stream, pos)[0] if b & 1 else b) >> 3
            code = (b >> 1) & 3
            body = c * T.ROW_BYTES[code]
            if c > row_end - row or pos + h + body > S or (c and n >= rec_end):
                raise IndexMismatch("COPY body")
            packets.append(("copy", T.unpack_rows(stream[pos + h : pos + h + body], c, code), code, bool(b & 1)))
            n += 1 if c else 0
            row += c
            pos += h + body
        rle = False
        if landed(RLE):
            return packets, pos, row, n
        if pos >= S:
            raise IndexMismatch("RLE header")
        b = stream[pos]
        h = 4 if b & 1 else 1
        if pos + h > S:
            raise IndexMismatch("RLE header")
        c = (struct.unpack_from("<I", stream, pos)[0] if b & 1 else b) >> 1
        if c == 0:
            pos += h
            if end is not None or row != R or pos + tail > S:
                raise IndexMismatch("end")
            packets.append(("rle", 0, None, bool(b & 1)))
            return packets, pos, row, n
        if c > row_end - row or pos + h + 1 > S or n >= rec_end:
            raise IndexMismatch("RLE")
        packets.append(("rle", c, stream[pos + h], bool(b & 1)))
        n += 1
        row += c
        pos += h + 1


def model_indexed_parse(stream, index):
    """The packet list of `stream` by the stretch walks of `index`: every entry checked before use (bounds; order behind the entry in front of it), every
    stretch ending on the next entry in exactly its state.  Raises T.Malformed for a stream header that is bad by itself, IndexMismatch for everything
    that makes index and stream disagree."""
    stream, index = bytes(stream), bytes(index)
    if len(stream) < 10:
        raise T.Malformed("short")
    in_size, S = struct.unpack_from("<II", stream, 0)
    if S > len(stream) or S < 10 or in_size == 0:
        raise T.Malformed("header")
    if len(index) < HEADER or index[:8] != MAGIC:
        raise IndexMismatch("index header")
    version, header, i_size, i_stream, spacing, count, size = struct.unpack_from("<IIIIIIQ", index, 8)
    if (version, header, i_size, i_stream, size) != (1, HEADER, in_size, S, HEADER + 16 * count) or len(index) < size or any(index[40:HEADER]):
        raise IndexMismatch("index header")
    R, tail = in_size // 16, in_size % 16
    max_rec = R + 1
    entries = [struct.unpack_from("<IIII", index, HEADER + 16 * k) for k in range(count)]
    prev = (8, 0, 0, COPY)
    for e in entries:
        off, row, n, kind = e
        if not (8 <= off < S and row < R and n < max_rec and n <= row and kind <= 1):
            raise IndexMismatch("entry out of bounds")
        if not (off > prev[0] and row > prev[1] and n > prev[2]):
            raise IndexMismatch("entries out of order")
        prev = e
    packets = []
    for k in range(count + 1):
        start = entries[k - 1] if k else (8, 0, 0, COPY)
        got, _, _, _ = _walk(stream, S, R, tail, start[0], start[1], start[2], start[3] == RLE, entries[k] if k < count else None, max_rec)
        packets += got
    return packets


# ---- streams ----

def _spec(spec, tail=b"", seed=1):
    return T.model_compress(T.data_from_rank_rows(T.rows_from_spec(spec, seed), tail))


def encoder_inputs():
    """name -> input bytes: the cases of the index (spacing 64 unless a test says otherwise), shaped by the packets they produce.  48 to ~400 rows."""
    c = {}
    f = lambda spec, tail=b"", seed=1: T.data_from_rank_rows(T.rows_from_spec(spec, seed), tail)
    c["no_entry"] = f([("copy", 10, 200), ("rle", 38, 0)])                                   # 48 rows: every packet begins in front of row 64
    c["entry_on_copy"] = f([("rle", 70, 1), ("copy", 30, 7), ("rle", 60, 0)], b"\x01")
    c["entry_on_rle_behind_copy"] = f([("copy", 70, 15), ("rle", 30, 2), ("copy", 50, 3)])
    c["entry_on_rle_behind_rle"] = f([("rle", 70, 1), ("rle", 60, 2), ("rle", 40, 1), ("copy", 3, 9)])
    c["begins_on_window_edge"] = f([("copy", 64, 3), ("rle", 64, 0), ("copy", 64, 7), ("rle", 1, 1)])            # packets that begin exactly on j * 64
    c["begins_on_window_last_row"] = f([("copy", 127, 3), ("rle", 64, 0), ("copy", 64, 7), ("rle", 2, 1)])       # ... on j * 64 + 63
    c["long_8bit_copy"] = f([("rle", 60, 0), ("copy", 75, 255), ("rle", 70, 3), ("copy", 5, 1)])                  # a body above the 1 KiB window; a window without entry
    c["long_rle"] = f([("copy", 5, 3), ("rle", 300, 0), ("copy", 40, 15), ("rle", 20, 1)], b"\x02" * 15)          # an RLE across several windows
    c["alternating_one_row_packets"] = f([("copy", 1, 100) if i % 2 == 0 else ("rle", 1, i % 5) for i in range(256)])
    c["uniform_first_row"] = f([("rle", 3, 0), ("copy", 80, 40), ("rle", 50, 1), ("rle", 20, 0)])                 # a first COPY of no rows
    c["ends_with_copy"] = f([("rle", 100, 0), ("copy", 60, 3)], b"\x05")
    c["under_one_row"] = bytes(range(7, 20))[:13]                                                                 # inSize < 16
    return c


def grammar_index_streams():
    """name -> stream: legal streams no encoder writes, with entries on their unusual packets at spacing 64."""
    rng = random.Random(77)
    end = ("rle", 0, None, False)
    lit = lambda k, top=3: T.literal_rows(k, top, rng)
    out = {}
    # an RLE behind an RLE: the null COPY in front in short and in 4-byte form
    out["null_copy_short_in_front_of_entry"] = (16 * 140, [("copy", [], 3, False), ("rle", 70, 1, False), ("copy", [], 0, False), ("rle", 70, 2, False), ("copy", [], 0, False), end], b"")
    out["null_copy_long_in_front_of_entry"] = (16 * 140, [("copy", [], 0, False), ("rle", 70, 1, False), ("copy", [], 2, True), ("rle", 70, 2, True), ("copy", [], 0, True), end], b"")
    # 4-byte headers with small counts on entries
    out["long_headers_on_entries"] = (16 * 150 + 3, [("copy", lit(66, 200), 0, True), ("rle", 3, 0, True), ("copy", lit(60, 3), 3, True), ("rle", 5, 1, True), ("copy", lit(16, 7), 2, True),
                                                     ("rle", 0, None, True)], b"\x01\x02\x03")
    # every terminator form with 0, 1 and 15 tail ranks
    for tail in (0, 1, 15):
        t = bytes(range(1, tail + 1))
        out[f"ends_copy_rle0_tail{tail}"] = (16 * 130 + tail, [("copy", lit(65, 15), 1, True), ("rle", 5, 0, False), ("copy", lit(60, 7), 2, True), end], t)
        out[f"ends_copy_long_rle0_tail{tail}"] = (16 * 130 + tail, [("copy", lit(65, 15), 1, True), ("rle", 5, 0, False), ("copy", lit(60, 7), 2, True), ("rle", 0, None, True)], t)
        out[f"ends_rle_nullcopy_rle0_tail{tail}"] = (16 * 130 + tail, [("copy", lit(65, 15), 1, True), ("rle", 65, 0, False), ("copy", [], 0, False), end], t)
        out[f"ends_rle_long_nullcopy_long_rle0_tail{tail}"] = (16 * 130 + tail, [("copy", lit(65, 15), 1, True), ("rle", 65, 0, False), ("copy", [], 1, True), ("rle", 0, None, True)], t)
    return {k: T.write_stream(n, packets, tail) for k, (n, packets, tail) in out.items()}


def restated_grammar_streams():
    """The grammar streams of test_gpu_rle8_mmtf.py, restated (a test file is not imported): legal streams no encoder writes."""
    rng = random.Random(21)
    end = ("rle", 0, None, False)
    out = {}
    for code in range(4):
        out[f"first_null_copy_code{code}"] = (48, [("copy", [], code, False), ("rle", 2, 5, False), ("copy", [], code, True), ("rle", 1, 5, False), ("copy", [], 0, False),
                                                   ("rle", 0, None, True)], b"")
        rows = T.literal_rows(7, 3, rng)
        out[f"long_copy_header_code{code}"] = (16 * 9 + 2, [("copy", rows, code, True), ("rle", 2, 0, True), ("copy", [], 0, False), end], b"\x07\x01")
        for k in (1, 4, 6, 13):
            rows = T.literal_rows(k, 3, rng) + [b"\x02" * 16]
            out[f"uniform_rows_in_copy_code{code}_{k + 1}"] = (16 * (k + 1), [("copy", rows, code, False), end], b"")
    lit = T.literal_rows(3, 200, rng)
    out["long_rle_headers"] = (16 * 30 + 1, [("copy", lit, 0, False), ("rle", 10, 2, True), ("copy", [], 0, False), ("rle", 7, 2, False), ("copy", [], 6 >> 1, False),
                                             ("rle", 5, 1, True), ("copy", [], 0, True), ("rle", 5, 0, False), ("copy", [], 0, False), end], b"\x09")
    out["rle_counts_above_rank_plus_one"] = (16 * 300, [("copy", [], 3, False), ("rle", 100, 3, False), ("copy", [], 0, False), ("rle", 130, 1, True), ("copy", [], 0, False),
                                                        ("rle", 70, 200, False), ("copy", [], 0, False), end], b"")
    return {k: T.write_stream(n, packets, tail) for k, (n, packets, tail) in out.items()}


def malformed_streams():
    """name -> (uncompressed size, stream): the malformed streams of test_gpu_rle8_mmtf.py, restated."""
    rng = random.Random(33)
    rows = T.literal_rows(6, 200, rng)
    end = ("rle", 0, None, False)
    good = T.write_stream(96, [("copy", rows, 0, False), end])
    return {
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


# ---- tampers ----

def tamper_base():
    """A stream with many entries of both kinds at spacing 64 (and a last window without one, so that one entry more is still a count the header may
    hold), and another stream of the same sizes and entry count whose packets lie elsewhere."""
    a = _spec([("copy", 70, 3), ("rle", 30, 2), ("rle", 60, 1), ("copy", 66, 7), ("rle", 64, 0), ("copy", 50, 3), ("rle", 108, 5)], b"\x03", seed=2)
    b = _spec([("copy", 70, 3), ("rle", 34, 2), ("rle", 56, 1), ("copy", 66, 7), ("rle", 60, 0), ("copy", 50, 3), ("rle", 112, 5)], b"\x03", seed=2)
    return a, b


def single_field_tampers(index):
    """name -> index bytes: every field of every entry +1 and -1, kind flipped and kind 2."""
    in_size, stream_size, spacing, entries = unpack_index(index)
    out = {}
    for k, e in enumerate(entries):
        for f, name in enumerate(("offset", "row", "ordinal")):
            for d in (1, -1):
                t = list(e)
                t[f] += d
                out[f"entry{k}_{name}{d:+d}"] = pack_index(in_size, stream_size, spacing, entries[:k] + [tuple(t)] + entries[k + 1 :])
        for kind in (1 - e[3], 2):
            out[f"entry{k}_kind{kind}"] = pack_index(in_size, stream_size, spacing, entries[:k] + [e[:3] + (kind,)] + entries[k + 1 :])
    return out


def structural_tampers(stream, index):
    """name -> index bytes: two entries swapped, one duplicated (over its neighbour, and inserted), one pointing into a body, the header's entryCount
    + 1 and - 1 (the count field alone: 16 bytes of zeros follow the entries for the + 1)."""
    in_size, stream_size, spacing, entries = unpack_index(index)
    assert len(entries) >= 3
    pack = lambda es: pack_index(in_size, stream_size, spacing, es)
    count = lambda d: index[:28] + struct.pack("<I", len(entries) + d) + index[32:] + bytes(16)
    out = {
        "swapped": pack([entries[1], entries[0]] + entries[2:]),
        "duplicated_over_neighbour": pack([entries[0], entries[0]] + entries[2:]),
        "duplicated_inserted": pack([entries[0], entries[0]] + entries[1:]),
        "count_plus_one": count(1),
        "count_minus_one": count(-1),
        "count_plus_one_zeros_entry": pack(entries + [(0, 0, 0, 0)]),
        "count_plus_one_copy_of_last": pack(entries + [entries[-1]]),
    }
    # into a body: the first COPY packet with a body behind an entry
    for k, (off, row, n, kind) in enumerate(entries):
        if kind == COPY:
            out["into_a_body"] = pack(entries[:k] + [(off + 2, row, n, kind)] + entries[k + 1 :])
            break
    assert "into_a_body" in out
    return out
