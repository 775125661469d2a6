"""Helpers of the rle8_mmtf128 tests (reference: src/rle8_mmtf.c, src/rle.h:442-452): a sequential model of the encoder (the reference's state
machine, with the start value of the first packet's OR mask defined as ZERO) and of the decoder, a grammar writer that builds streams packet by
packet, a parser that gives the packet list back, a ctypes wrapper of the compiled reference (optional: oracle/_ref/libhsrle_ref.so), and inputs.

Stream: u32 inSize, u32 streamSize, COPY / RLE packets in turn (COPY first), the chain ends at an RLE header of count 0, then inSize % 16 tail ranks.
  COPY  c rows:  c << 3 | code << 1 (one byte, c < 32)  or  u32 c << 3 | 1 | code << 1;  code 0 = 8 bit rows, 1 = 4 bit, 2 = 3 bit, 3 = 2 bit
  RLE   c rows of rank s:  c << 1, s (c < 128)  or  u32 c << 1 | 1, s
"""
import ctypes
import os
import random
import struct

from mmtf_testlib import mmtf_dec, mmtf_enc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(REPO, "oracle", "_ref", "libhsrle_ref.so")
GOLDEN = os.path.join(REPO, "tests", "golden", "rle8_mmtf", "vectors.json")

ROW_BYTES = {0: 16, 1: 8, 2: 6, 3: 4}     # body bytes per row of a width code
CODE_MAX = {0: 255, 1: 15, 2: 7, 3: 3}    # largest rank a width code holds


class Malformed(Exception):
    pass


def width_code(or_byte):
    """The reference's order: hi-4, then hi-6, then hi-5 (rle8_mmtf.c:257-288)."""
    if or_byte & 0xF0:
        return 0
    if not or_byte & 0xFC:
        return 3
    return 2 if not or_byte & 0xF8 else 1


def rows_or(rows):
    m = 0
    for r in rows:
        for b in r:
            m |= b
    return m


def is_uniform(row):
    return row == row[:1] * 16


# ---- bodies ----

def _mask(row, bit, shift=0):
    return sum(((row[j] >> bit) & 1) << (j + shift) for j in range(16))


def pack_rows(rows, code):
    c = len(rows)
    assert rows_or(rows) <= CODE_MAX[code], "a row does not fit the width"
    out = bytearray()
    if code == 0:
        for r in rows:
            out += r
    elif code == 1:       # pairs: first row << 4 | second row; a last single row: bytes 0-7 | bytes 8-15 << 4
        for k in range(0, c - 1, 2):
            out += bytes(a << 4 | b for a, b in zip(rows[k], rows[k + 1]))
        if c & 1:
            r = rows[-1]
            out += bytes(r[j] | r[8 + j] << 4 for j in range(8))
    elif code == 3:       # groups of 4 rows in 16 bytes; then a dword per row
        full = c // 4 * 4
        for k in range(0, full, 4):
            out += bytes(rows[k][j] | rows[k + 1][j] << 2 | rows[k + 2][j] << 4 | rows[k + 3][j] << 6 for j in range(16))
        for r in rows[full:]:
            out += bytes(r[j] | r[4 + j] << 2 | r[8 + j] << 4 | r[12 + j] << 6 for j in range(4))
    else:                 # groups of 6 rows in 36 bytes; then three 16 bit masks per row
        full = c // 6 * 6
        for k in range(0, full, 6):
            p = rows[k : k + 6]
            out += bytes(p[0][j] | p[1][j] << 3 | (p[2][j] & 3) << 6 for j in range(16))
            out += bytes(p[3][j] | p[4][j] << 3 | (p[5][j] & 3) << 6 for j in range(16))
            out += struct.pack("<I", _mask(p[2], 2) | _mask(p[5], 2, 16))
        for r in rows[full:]:
            out += struct.pack("<HHH", _mask(r, 0), _mask(r, 1), _mask(r, 2))
    assert len(out) == c * ROW_BYTES[code]
    return bytes(out)


def _spread(m):
    return [(m >> j) & 1 for j in range(16)]


def unpack_rows(body, c, code):
    rows = []
    if code == 0:
        return [bytes(body[16 * i : 16 * i + 16]) for i in range(c)]
    if code == 1:
        for k in range(c // 2):
            g = body[16 * k : 16 * k + 16]
            rows.append(bytes(b >> 4 for b in g))
            rows.append(bytes(b & 15 for b in g))
        if c & 1:
            g = body[8 * (c - 1) : 8 * (c - 1) + 8]
            rows.append(bytes(b & 15 for b in g) + bytes(b >> 4 for b in g))
    elif code == 3:
        full = c // 4 * 4
        for i in range(full):
            g = body[16 * (i // 4) : 16 * (i // 4) + 16]
            rows.append(bytes((b >> 2 * (i % 4)) & 3 for b in g))
        for i in range(full, c):
            g = body[4 * i : 4 * i + 4]
            rows.append(bytes((g[j % 4] >> 2 * (j // 4)) & 3 for j in range(16)))
    else:
        full = c // 6 * 6
        for k in range(0, full, 6):
            g = body[6 * k : 6 * k + 36]
            (m25,) = struct.unpack_from("<I", g, 32)
            for half, m in ((g[:16], m25 & 0xFFFF), (g[16:32], m25 >> 16)):
                rows.append(bytes(b & 7 for b in half))
                rows.append(bytes((b >> 3) & 7 for b in half))
                rows.append(bytes((b >> 6) | s << 2 for b, s in zip(half, _spread(m))))
        for i in range(full, c):
            m0, m1, m2 = struct.unpack_from("<HHH", body, 6 * i)
            rows.append(bytes(a | b << 1 | d << 2 for a, b, d in zip(_spread(m0), _spread(m1), _spread(m2))))
    return rows


# ---- the grammar writer ----
# packets: ("copy", [rows], code, long_header) and ("rle", count, rank, long_header), in stream order; the writer adds nothing by itself: the caller
# writes null COPYs (("copy", [], code, long)) and the ending null RLE (("rle", 0, None, long)) where the grammar wants them.

def write_packet(p):
    if p[0] == "copy":
        _, rows, code, long_header = p
        c = len(rows)
        assert long_header or c < 32
        head = struct.pack("<I", c << 3 | 1 | code << 1) if long_header else bytes([c << 3 | code << 1])
        return head + pack_rows(rows, code)
    _, c, rank, long_header = p
    assert long_header or c < 128
    head = struct.pack("<I", c << 1 | 1) if long_header else bytes([c << 1])
    return head + (bytes([rank]) if c else b"")


def write_stream(in_size, packets, tail_ranks=b"", stream_size=None):
    chain = b"".join(write_packet(p) for p in packets) + bytes(tail_ranks)
    return struct.pack("<II", in_size, 8 + len(chain) if stream_size is None else stream_size) + chain


def parse_stream(stream, out_cap=None):
    """(in_size, packets with the rows unpacked, ranks).  Raises Malformed exactly where the library says malformed: a packet past streamSize or
    past the last row, a chain not ended when the rows are used up, rows left over, a tail past streamSize."""
    stream = bytes(stream)
    if len(stream) < 10:
        raise Malformed("short")
    in_size, S = struct.unpack_from("<II", stream, 0)
    if S > len(stream) or S < 10 or in_size == 0 or (out_cap is not None and in_size > out_cap):
        raise Malformed("header")
    R, tail = in_size // 16, in_size % 16
    pos, row, packets, ranks = 8, 0, [], bytearray()
    while True:
        if pos >= S:
            raise Malformed("COPY header")
        b = stream[pos]
        h = 4 if b & 1 else 1
        if pos + h > S:
            raise Malformed("COPY header")
        c = (struct.unpack_from("<I", stream, pos)[0] if b & 1 else b) >> 3
        code = (b >> 1) & 3
        body = c * ROW_BYTES[code]
        if c > R - row or pos + h + body > S:
            raise Malformed("COPY body")
        rows = unpack_rows(stream[pos + h : pos + h + body], c, code)
        packets.append(("copy", rows, code, bool(b & 1)))
        for r in rows:
            ranks += r
        row += c
        pos += h + body
        if pos >= S:
            raise Malformed("RLE header")
        b = stream[pos]
        h = 4 if b & 1 else 1
        if pos + h > S:
            raise Malformed("RLE header")
        c = (struct.unpack_from("<I", stream, pos)[0] if b & 1 else b) >> 1
        if c == 0:
            packets.append(("rle", 0, None, bool(b & 1)))
            pos += h
            break
        if c > R - row or pos + h + 1 > S:
            raise Malformed("RLE")
        packets.append(("rle", c, stream[pos + h], bool(b & 1)))
        ranks += bytes([stream[pos + h]]) * (16 * c)
        row += c
        pos += h + 1
    if row != R or pos + tail > S:
        raise Malformed("end")
    ranks += stream[pos : pos + tail]
    return in_size, packets, bytes(ranks)


# ---- the model ----

def encode_packets(ranks):
    """The reference's encoder state machine (rle8_mmtf.c:190-626) over the rank rows, start mask zero: the packet list as the writer takes it."""
    R = len(ranks) // 16
    packets = []
    copying, count, mask, rows, symbol = True, 0, 0, [], 0

    def end_copy():
        packets.append(("copy", list(rows), width_code(mask), len(rows) >= 32))

    def end_rle():
        packets.append(("rle", count, symbol, count >= 128))

    for i in range(R):
        out = ranks[16 * i : 16 * i + 16]
        if copying:
            if is_uniform(out):
                end_copy()
                copying, symbol, count = False, out[0], 1
            else:
                mask |= rows_or([out])
                rows.append(out)
                count += 1
        elif is_uniform(out) and out[0] == symbol:
            count += 1
        else:
            end_rle()
            if is_uniform(out):
                packets.append(("copy", [], 0, False))     # the null COPY between two RLE packets: byte 0x00
                symbol, count = out[0], 1
            else:
                copying, rows, mask, count = True, [out], rows_or([out]), 1
    if copying:
        end_copy()
        packets.append(("rle", 0, None, False))
    else:
        end_rle()
        packets.append(("copy", [], 0, False))
        packets.append(("rle", 0, None, False))
    return packets


def model_compress(data):
    data = bytes(data)
    ranks = mmtf_enc(data, 16)
    R = len(data) // 16
    return write_stream(len(data), encode_packets(ranks), ranks[16 * R :])


def model_decompress(stream, out_cap=None):
    """The decoded bytes, or None for a malformed stream."""
    try:
        _, _, ranks = parse_stream(stream, out_cap)
    except Malformed:
        return None
    return mmtf_dec(ranks, 16)


def first_copy_end(stream):
    """Offset behind the first COPY packet."""
    b = stream[8]
    h = 4 if b & 1 else 1
    c = (struct.unpack_from("<I", stream, 8)[0] if b & 1 else b) >> 3
    return 8 + h + c * ROW_BYTES[(b >> 1) & 3]


def reference_is_deterministic(data):
    """Row 0 is not uniform and a row of the first COPY packet holds a rank >= 16: the undefined start value cannot change the reference's stream."""
    ranks = mmtf_enc(bytes(data), 16)
    for i in range(len(data) // 16):
        row = ranks[16 * i : 16 * i + 16]
        if is_uniform(row):
            return False
        if max(row) >= 16:
            return True
    return False


def local_rule_packets(ranks):
    """The packet structure by the LOCAL rule (no carried state): (kind, count, rank) with the null packets, to hold against a parsed stream."""
    R = len(ranks) // 16
    rows = [ranks[16 * i : 16 * i + 16] for i in range(R)]
    out, i = [], 0
    if R == 0 or is_uniform(rows[0]):
        out.append(("copy", 0, None))
    last = "copy"
    while i < R:
        j = i + 1
        if is_uniform(rows[i]):
            while j < R and rows[j] == rows[i]:
                j += 1
            if last == "rle":
                out.append(("copy", 0, None))
            out.append(("rle", j - i, rows[i][0]))
            last = "rle"
        else:
            while j < R and not is_uniform(rows[j]):
                j += 1
            out.append(("copy", j - i, None))
            last = "copy"
        i = j
    if last == "rle" and R:
        out.append(("copy", 0, None))
    out.append(("rle", 0, None))
    return out


def structure(packets):
    return [("copy", len(p[1]), None) if p[0] == "copy" else ("rle", p[1], p[2]) for p in packets]


# ---- the compiled reference ----

class Rle8MmtfReference:
    @staticmethod
    def available():
        return os.path.exists(REF_LIB)

    def __init__(self):
        self.lib = ctypes.CDLL(REF_LIB)
        for nm in ("rle8_mmtf128_compress", "rle8_mmtf128_decompress"):
            f = getattr(self.lib, nm)
            f.restype = ctypes.c_uint32
            f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
        for nm in ("rle8_mmtf128_compress_bounds", "rle8_mmtf256_compress_bounds"):
            f = getattr(self.lib, nm)
            f.restype = ctypes.c_uint32
            f.argtypes = [ctypes.c_uint32]

    def bounds(self, n, name="rle8_mmtf128_compress_bounds"):
        return getattr(self.lib, name)(n)

    def compress(self, data):
        """The reference's stream.  (Its bound is 5 bytes short for incompressible input and it writes past it: the buffer has slack.)"""
        data = bytes(data)
        dst = ctypes.create_string_buffer(len(data) + 256)
        n = self.lib.rle8_mmtf128_compress(data, len(data), dst, len(data) + 64)
        return dst.raw[:n]

    def decompress(self, stream, out_size):
        stream = bytes(stream)
        src = ctypes.create_string_buffer(stream + bytes(64), len(stream) + 64)
        dst = ctypes.create_string_buffer(out_size + 256)
        n = self.lib.rle8_mmtf128_decompress(src, len(stream), dst, out_size)
        return n, dst.raw[:n]


# ---- inputs ----

def data_from_rank_rows(rows, tail=b""):
    """The input whose mmtf128 ranks are exactly `rows` (+ tail ranks): the tests shape the PACKETS they want and get the bytes from the inverse."""
    return mmtf_dec(b"".join(rows) + bytes(tail), 16)


def literal_rows(count, top, rng):
    """`count` non-uniform rows of ranks <= top; their OR is exactly the bits of `top`'s width (the first row holds `top`)."""
    rows = []
    for i in range(count):
        r = bytearray(rng.randrange(top + 1) for _ in range(16))
        if i == 0:
            r[3] = top
        r[0], r[1] = (0, 1) if r[0] == r[1] else (r[0], r[1])   # never uniform
        rows.append(bytes(r))
    return rows


def rows_from_spec(spec, seed=1):
    """spec: list of ("rle", count, rank) / ("copy", count, top rank).  Neighbouring entries must differ in kind or rank to stay separate packets."""
    rng = random.Random(seed)
    rows = []
    for kind, count, v in spec:
        rows += [bytes([v]) * 16] * count if kind == "rle" else literal_rows(count, v, rng)
    return rows


def random_alphabet(n, alphabet, seed, run=1):
    """Random bytes over `alphabet` symbols, each drawn symbol repeated over `run` whole rows with probability 1/2 (so that uniform rows occur)."""
    rng = random.Random(seed * 7919 + alphabet * 131 + n)
    out = bytearray()
    while len(out) < n:
        if rng.random() < 0.5:
            out += bytes([rng.randrange(alphabet)]) * (16 * rng.randrange(1, 4 * run + 1))
        else:
            out += bytes(rng.randrange(alphabet) for _ in range(16 * rng.randrange(1, 4)))
    return bytes(out[:n])
