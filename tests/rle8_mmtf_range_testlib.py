"""Helpers of the tests of the rle8_mmtf128 checkpoints and byte-range decode (include/hsrle.h section 5; csrc/hsrle_rle8mmtf_range.hip.h), on top of
rle8_mmtf_testlib (the stream), rle8_mmtf_index_testlib (the entry index and its stretch walk) and mmtf_testlib (the transform): the checkpoint sidecar
from the sequential definition of mmtf128, and the range decode step by step as the device does it.

Checkpoints: 64 header bytes ("HSRLEMFC", u32 version 1, u32 headerBytes 64, u32 uncompressedSize, u32 streamSize, u32 checkpointRows, u32 checkpointCount,
u64 size, zeros), then per k = 1 .. checkpointCount the sixteen lists in front of row k * checkpointRows, 256 bytes each, byte i = the symbol of rank i.
"""
import bisect
import struct

import rle8_mmtf_index_testlib as X
import rle8_mmtf_testlib as T

MAGIC = b"HSRLEMFC"
HEADER = 64
CHECKPOINT = 4096
CHECKPOINT_ROWS = (64, 128)
DONE, MALFORMED, CAPACITY, INDEX, CHECKPOINT_STATUS = 0, 1, 2, 3, 4


class CheckpointMismatch(Exception):
    pass


def checkpoint_count(in_size, checkpoint_rows):
    rows = in_size // 16
    return (rows - 1) // checkpoint_rows if rows else 0


def pack_checkpoints(in_size, stream_size, checkpoint_rows, checkpoints):
    """checkpoints: per checkpoint the sixteen lists (sequences of 256 symbols)"""
    head = MAGIC + struct.pack("<IIIIIIQ", 1, HEADER, in_size, stream_size, checkpoint_rows, len(checkpoints), HEADER + CHECKPOINT * len(checkpoints))
    return head + bytes(HEADER - len(head)) + b"".join(bytes(l) for lists in checkpoints for l in lists)


def unpack_checkpoints(sidecar):
    """(in_size, stream_size, checkpoint_rows, [per checkpoint its sixteen lists as bytes]) of sidecar bytes whose header is taken on trust"""
    version, header, in_size, stream_size, rows, count, size = struct.unpack_from("<IIIIIIQ", sidecar, 8)
    assert sidecar[:8] == MAGIC and (version, header, size) == (1, HEADER, HEADER + CHECKPOINT * count) and len(sidecar) >= size
    at = lambda k, c: HEADER + CHECKPOINT * k + 256 * c
    return in_size, stream_size, rows, [[sidecar[at(k, c) : at(k, c) + 256] for c in range(16)] for k in range(count)]


def lists_in_front_of(data, rows):
    """the sixteen lists of mmtf128 in front of each row of `rows` (ascending), by the sequential definition"""
    lists = [list(range(256)) for _ in range(16)]
    out, done = [], 0
    for row in rows:
        for i in range(16 * done, 16 * row):
            l = lists[i % 16]
            k = l.index(data[i])
            if k:
                l.insert(0, l.pop(k))
        done = row
        out.append([list(l) for l in lists])
    return out


def model_checkpoints(data, checkpoint_rows, stream_size=None):
    """the sidecar of `data`; stream_size: the header's word (None: the size of the model's own stream of data)"""
    data = bytes(data)
    count = checkpoint_count(len(data), checkpoint_rows)
    size = len(T.model_compress(data)) if stream_size is None else stream_size
    return pack_checkpoints(len(data), size, checkpoint_rows, lists_in_front_of(data, [k * checkpoint_rows for k in range(1, count + 1)]))


def range_rows(in_size, offset, length, checkpoint_rows):
    """(c, r1): the rows [c, r1) a range decode expands.  c is the last checkpoint row at or in front of the range's first row -- of the LAST row for a
    range of tail bytes alone, which is decoded through row R --, r1 the row behind the range's last byte, R at the most."""
    R = in_size // 16
    first = min(offset // 16, R - 1) if R else 0
    return first // checkpoint_rows * checkpoint_rows, min(R, (offset + length + 15) // 16)


def model_range_decode(stream, index, checkpoints, offset, length):
    """Output bytes [offset, offset + length) of `stream` the way the device finds them: the three headers against each other, the checkpoint of row c a set
    of sixteen permutations, e0 = the last entry with row <= c by binary search, the stretch walks from e0 with their entry checks, record bound and landing
    checks up to the stretch that reaches r1, the ranks of rows [c, r1), the lists from the checkpoint.  Raises T.Malformed, X.IndexMismatch or
    CheckpointMismatch where the device says MALFORMED, INDEX or CHECKPOINT."""
    stream, index, checkpoints = bytes(stream), bytes(index), bytes(checkpoints)
    if len(stream) < 10:
        raise T.Malformed("short")
    in_size, S = struct.unpack_from("<II", stream, 0)
    if S > len(stream) or S < 10 or in_size == 0:
        raise T.Malformed("header")
    if len(index) < X.HEADER or index[:8] != X.MAGIC:
        raise X.IndexMismatch("index header")
    version, header, i_size, i_stream, spacing, count, size = struct.unpack_from("<IIIIIIQ", index, 8)
    if (version, header, i_size, i_stream, size) != (1, X.HEADER, in_size, S, X.HEADER + 16 * count) or len(index) < size or any(index[40 : X.HEADER]):
        raise X.IndexMismatch("index header")
    if len(checkpoints) < HEADER or checkpoints[:8] != MAGIC:
        raise CheckpointMismatch("checkpoint header")
    version, header, c_size, c_stream, ck_rows, ck_count, size = struct.unpack_from("<IIIIIIQ", checkpoints, 8)
    if ck_rows % 64 or not 64 <= ck_rows <= 1 << 24:
        raise CheckpointMismatch("checkpoint rows")
    if (version, header, c_size, c_stream, ck_count, size) != (1, HEADER, in_size, S, checkpoint_count(in_size, ck_rows), HEADER + CHECKPOINT * ck_count) or len(checkpoints) < size \
            or any(checkpoints[40:HEADER]):
        raise CheckpointMismatch("checkpoint header")
    assert length > 0 and offset + length <= in_size
    R, tail = in_size // 16, in_size % 16
    c, r1 = range_rows(in_size, offset, length, ck_rows)
    lists = [list(range(256)) for _ in range(16)]
    if c:
        lists = [list(l) for l in unpack_checkpoints(checkpoints)[3][c // ck_rows - 1]]
        if any(sorted(l) != list(range(256)) for l in lists):
            raise CheckpointMismatch("not a permutation")
    entries = [struct.unpack_from("<IIII", index, X.HEADER + 16 * k) for k in range(count)]
    origin = (8, 0, 0, X.COPY)
    in_bounds = lambda e: 8 <= e[0] < S and e[1] < R and e[2] < R + 1 and e[2] <= e[1] and e[3] <= 1
    k0 = bisect.bisect_right([e[1] for e in entries], c)             # stretch k0 starts at entry k0 - 1; 0: the chain's start
    e0 = entries[k0 - 1] if k0 else origin
    cap = (r1 - c) + 2 * spacing + 1
    if (k0 and not in_bounds(e0)) or e0[1] > c:
        raise X.IndexMismatch("e0")
    rows, reached, tail_at = {}, False, None
    for i in range((r1 - c) // spacing + 3):
        k = k0 + i
        if k > count:
            break
        start = entries[k - 1] if k else origin
        if i and start[1] >= r1:
            break
        last = k == count
        if i and not (in_bounds(start) and 0 <= start[2] - e0[2] <= cap):
            raise X.IndexMismatch("entry")
        end = None if last else entries[k]
        if end is not None and not (in_bounds(end) and end[0] > start[0] and end[1] > start[1] and end[2] > start[2] and end[2] - e0[2] <= cap):
            raise X.IndexMismatch("next entry")
        packets, pos, row, n = X._walk(stream, S, R, tail, start[0], start[1], start[2], start[3] == X.RLE, end, e0[2] + cap)
        at = start[1]
        for p in packets:
            for r in (p[1] if p[0] == "copy" else [bytes([p[2]]) * 16] * p[1] if p[1] else []):   # (the chain's last RLE has no rows and no rank)
                rows[at] = r
                at += 1
        if last or end[1] >= r1:
            reached, tail_at = True, pos if last else None
            break
    if not reached:
        raise X.IndexMismatch("the stretches do not reach the range's end")
    out = bytearray()
    for r in range(c, r1):
        for col in range(16):
            l = lists[col]
            k = rows[r][col]
            out.append(l[k])
            if k:
                l.insert(0, l.pop(k))
    if r1 == R:
        out += bytes(lists[j][stream[tail_at + j]] for j in range(tail))
    return bytes(out[offset - 16 * c : offset - 16 * c + length])


def range_grid(n):
    """(offset, length) of the range tests for an input of n bytes: around a row, a window of 64 rows, 128 rows, the end; short, a row, 1 KiB, to the end"""
    offsets = [o for o in (0, 1, 15, 16, 17, 16 * 64 - 1, 16 * 64, 16 * 64 + 1, 16 * 128, n - 17, n - 16, n - 1) if 0 <= o < n]
    out = []
    for o in offsets:
        for length in (1, 15, 16, 17, 1024, n - o):
            length = min(length, n - o)
            if (o, length) not in out:
                out.append((o, length))
    return out


def range_streams():
    """name -> (stream, its input): every stream of the index's cases, the encoder's and the grammar-written"""
    out = {}
    for name, data in X.encoder_inputs().items():
        out[name] = (T.model_compress(data), data)
    for name, stream in X.grammar_index_streams().items():
        out[name] = (stream, T.model_decompress(stream))
    return out


def mixed_input(rows=2000, seed=9):
    """about `rows` rows of mixed packets: literal stretches of every width, short and long runs, runs behind runs, a tail"""
    import random

    rng = random.Random(seed)
    spec, have = [], 0
    while have < rows:
        kind = rng.randrange(4)
        if kind == 0:
            item = ("copy", rng.randrange(1, 90), rng.choice((3, 7, 15, 255)))
        elif kind == 1:
            item = ("rle", rng.randrange(1, 200), rng.randrange(4))
        elif kind == 2:
            item = ("rle", rng.randrange(1, 8), rng.randrange(30))
        else:
            item = ("copy", rng.randrange(1, 6), 255)
        spec.append(item)
        have += item[1]
    return T.data_from_rank_rows(T.rows_from_spec(spec, seed), b"\x01\x00\x07")
