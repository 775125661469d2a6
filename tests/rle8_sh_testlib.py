"""Helpers of the rle8_sh tests (reference: src/rle_sh.c, src/rle.h:455-458): a sequential model of the decoder (the reference's, u32 wrap included,
with the library's refusal rules), a stream writer from a token list, two models of the encoder (the reference's byte loop restated, and the same
decisions as a loop over maximal runs of equal bytes), a ctypes wrapper of the compiled reference (optional: oracle/_ref/libhsrle_ref.so), inputs.

Stream: u32 inSize, u32 streamSize, a body of whole bytes upward from offset 8, a bit stream downward from the last byte (bit k of it is bit k % 8
of byte streamSize - 1 - k / 8).  Tokens, LSB first:
  Z 0 (the run symbol R)   L 10 (one body byte)   S 110 (second)   T 1110 (third)   FILL small 11110 (body u8 + 14 bytes of R)
  11111 00 raw COPY small (body u8 + 7 bytes)     11111 10 raw COPY large (body u32 + 7 bytes; a stored 0 ends the stream)
  11111 01 FILL large (body u32, new R; count = (stored + 14) mod 2^32)     11111 11 ENCODED COPY (body u8 + 161 symbols: Z / L / S, T as 111)
Token lists of the writer: ("Z",) ("L", byte) ("S",) ("T",) ("FILL", count) ("FILLL", stored u32, new R) ("COPY", bytes) ("COPYL", bytes)
("ENC", [symbol tokens]) ("END",).
"""
import ctypes
import os
import random
import struct

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(REPO, "oracle", "_ref", "libhsrle_ref.so")
GOLDEN = os.path.join(REPO, "tests", "golden", "rle8_sh", "vectors.json")

INIT_R, INIT_LAST, INIT_SECOND, INIT_THIRD = 0x7F, 0x80, 0x80, 0x7E
MIN_STREAM = 13          # header, the terminator's u32, one bit byte
MAX_IN = 1 << 30


class Malformed(Exception):
    pass


# ---- the writer ----

class _Out:
    def __init__(self):
        self.body = bytearray()
        self.nbits = 0
        self._chunks, self._acc, self._n = [], 0, 0      # whole 512-byte pieces of the bit stream (upward order), the bits behind them

    def put(self, value, count):
        self._acc |= value << self._n
        self._n += count
        self.nbits += count
        if self._n >= 4096:
            self._chunks.append((self._acc & ((1 << 4096) - 1)).to_bytes(512, "little"))
            self._acc >>= 4096
            self._n -= 4096

    def bit_bytes(self):
        """The bit stream's bytes in stream order (the byte of bits 0-7 last)."""
        up = b"".join(self._chunks) + self._acc.to_bytes((self._n + 7) // 8, "little")
        return up[::-1]

    def stream(self, in_size, gap=0, stream_size=None, gap_byte=0xA5):
        tail = self.bit_bytes()
        size = 8 + len(self.body) + gap + len(tail)
        return struct.pack("<II", in_size, size if stream_size is None else stream_size) + bytes(self.body) + bytes([gap_byte]) * gap + tail


def _put_symbol(o, t, enc):
    if t[0] == "Z":
        o.put(0b0, 1)
    elif t[0] == "L":
        o.put(0b01, 2)
        o.body.append(t[1])
    elif t[0] == "S":
        o.put(0b011, 3)
    elif t[0] == "T":
        o.put(0b111, 3) if enc else o.put(0b0111, 4)
    else:
        raise ValueError(t)


def write_stream(in_size, tokens, gap=0, stream_size=None):
    """The stream of a token list, written as it stands: nothing is checked, so that streams no encoder writes (and malformed ones) can be built."""
    o = _Out()
    for t in tokens:
        k = t[0]
        if k in "ZLST":
            _put_symbol(o, t, False)
        elif k == "FILL":
            o.put(0b01111, 5)
            o.body.append(t[1] - 14)
        elif k == "FILLL":
            o.put(0b1011111, 7)
            o.body += struct.pack("<I", t[1] & 0xFFFFFFFF)
            o.body.append(t[2])
        elif k == "COPY":
            o.put(0b0011111, 7)
            o.body.append(len(t[1]) - 7)
            o.body += t[1]
        elif k == "COPYL":
            o.put(0b0111111, 7)
            o.body += struct.pack("<I", len(t[1]) - 7)
            o.body += t[1]
        elif k == "ENC":
            o.put(0b1111111, 7)
            o.body.append(len(t[1]) - 161)
            for s in t[1]:
                _put_symbol(o, s, True)
        elif k == "END":
            o.put(0b0111111, 7)
            o.body += struct.pack("<I", 0)
        else:
            raise ValueError(t)
    return o.stream(in_size, gap, stream_size)


# ---- the decoder ----

def parse_stream(stream, stream_cap=None):
    """(inSize, token list, output) of a well-formed stream; Malformed by the library's rules (include/hsrle.h).  The decoding itself is the
    reference's: promotion at a literal equal to lastOccurred, FILL large counts mod 2^32."""
    stream = bytes(stream)
    cap = len(stream) if stream_cap is None else stream_cap
    if cap < MIN_STREAM:
        raise Malformed("stream shorter than header + terminator + one bit byte")
    n, S = struct.unpack_from("<II", stream, 0)
    if S > cap or S < MIN_STREAM or n == 0 or n > MAX_IN:
        raise Malformed("header sizes")
    R, last, second, third = INIT_R, INIT_LAST, INIT_SECOND, INIT_THIRD
    bit, body = 0, 8
    out, tokens = bytearray(), []

    def peek(k):
        idx = S - 1 - ((bit + k) >> 3)
        return (stream[idx] >> ((bit + k) & 7)) & 1 if idx >= 0 else 0

    def apart():
        if body + (bit + 7) // 8 > S:
            raise Malformed("body and bits meet")

    def symbol(enc):
        nonlocal bit, body, last, second, third
        if not peek(0):
            bit += 1
            out.append(R)
            return ("Z",)
        if not peek(1):
            bit += 2
            apart()
            v = stream[body]
            body += 1
            if v == last:
                third, second = second, v
            last = v
            out.append(v)
            return ("L", v)
        if not peek(2):
            bit += 3
            last = second
            out.append(second)
            return ("S",)
        bit += 3 if enc else 4
        last = third
        out.append(third)
        return ("T",)

    def u8():
        nonlocal body
        body += 1
        apart()
        return stream[body - 1]

    def u32():
        nonlocal body
        body += 4
        apart()
        return struct.unpack_from("<I", stream, body - 4)[0]

    while True:
        ones = 0
        while ones < 5 and peek(ones):
            ones += 1
        if ones < 4:
            tokens.append(symbol(False))
        elif ones == 4:
            bit += 5
            c = u8() + 14
            tokens.append(("FILL", c))
            out += bytes([R]) * c
        else:
            kind = peek(5) | peek(6) << 1
            bit += 7
            if kind == 0 or kind == 1:
                if kind == 0:
                    c = u8() + 7
                else:
                    c = u32()
                    if c == 0:
                        apart()
                        if len(out) != n:
                            raise Malformed("terminator with output missing")
                        tokens.append(("END",))
                        return n, tokens, bytes(out)
                    c += 7
                if len(out) + c > n:
                    raise Malformed("copy passes inSize")
                body += c
                apart()
                tokens.append(("COPY" if kind == 0 else "COPYL", stream[body - c : body]))
                out += stream[body - c : body]
            elif kind == 2:
                stored = u32()
                R = u8()
                if len(out) == n:
                    raise Malformed("a token behind the last output byte")
                c = (stored + 14) & 0xFFFFFFFF
                tokens.append(("FILLL", stored, R))
                if len(out) + c > n:
                    raise Malformed("fill passes inSize")
                out += bytes([R]) * c
            else:
                c = u8() + 161
                if len(out) + c > n:
                    raise Malformed("encoded copy passes inSize")
                tokens.append(("ENC", [symbol(True) for _ in range(c)]))
        apart()
        if len(out) > n:
            raise Malformed("output passes inSize")


def model_decompress(stream, stream_cap=None):
    """The decoded bytes, or None for a malformed stream."""
    try:
        return parse_stream(stream, stream_cap)[2]
    except Malformed:
        return None


# ---- the encoder: the reference's byte loop (rle_sh.c:269-505), restated ----

class _Enc:
    def __init__(self, data):
        self.d = data
        self.o = _Out()
        self.R, self.last, self.second, self.third = INIT_R, INIT_LAST, INIT_SECOND, INIT_THIRD
        self.items = []          # what was decided, for the tests: (kind, input offset, count)

    def symbols(self, start, count, enc):
        o = self.o
        for v in self.d[start : start + count]:
            if v == self.R:
                o.put(0b0, 1)
            elif v == self.second:
                o.put(0b011, 3)
                self.last = v
            elif v == self.third:
                o.put(0b111, 3) if enc else o.put(0b0111, 4)
                self.last = v
            else:
                o.put(0b01, 2)
                if v == self.last:
                    self.third, self.second = self.second, v
                self.last = v
                o.body.append(v)

    def copy(self, start, count):
        o = self.o
        if count > 255 + 7:
            self.items.append(("raw", start, count))
            o.put(0b0111111, 7)
            o.body += struct.pack("<I", count - 7)
            o.body += self.d[start : start + count]
        elif count >= 7:
            self.items.append(("raw", start, count))
            o.put(0b0011111, 7)
            o.body.append(count - 7)
            o.body += self.d[start : start + count]
        elif count:
            self.items.append(("sym", start, count))
            self.symbols(start, count, False)

    def encoded_copy(self, start, count):
        o = self.o
        while count:
            if count > 161:
                stored = min(0xFF, count - 161)
                c = stored + 161
                self.items.append(("enc", start, c))
                o.put(0b1111111, 7)
                o.body.append(stored)
                self.symbols(start, c, True)
                count -= c
                start += c
            else:
                self.items.append(("sym", start, count))
                self.symbols(start, count, False)
                return

    def block(self, start, count, r_bytes):
        """The `7 : 2` rule: a block with enough bytes of R in it is coded symbol by symbol."""
        if ((r_bytes * 7) & (2**64 - 1)) > (((count - r_bytes) * 2) & (2**64 - 1)):
            self.encoded_copy(start, count)
        else:
            self.copy(start, count)

    def fill(self, start, count):
        o = self.o
        if count > 255 + 14:
            self.items.append(("fill", start, count))
            o.put(0b1011111, 7)
            o.body += struct.pack("<I", count - 14)
            o.body.append(self.R)
        elif count >= 14:
            self.items.append(("fill", start, count))
            o.put(0b01111, 5)
            o.body.append(count - 14)
        elif count:
            self.items.append(("sym", start, count))
            o.put(0, count)

    def change(self, start, count, sym):
        self.items.append(("change", start, count))
        self.R = sym
        self.o.put(0b1011111, 7)
        self.o.body += struct.pack("<I", (count - 14) & 0xFFFFFFFF)
        self.o.body.append(sym)

    def finish(self):
        self.o.put(0b0111111, 7)
        self.o.body += struct.pack("<I", 0)
        return self.o.stream(len(self.d))


def model_compress_bytewise(data):
    """The reference's state machine byte by byte, names as in rle_sh.c."""
    data = bytes(data)
    assert data
    e = _Enc(data)
    lastSymbol, copyCount, rleChangeCount, rleCount, rleSymbolCopyCount = 0, 0, 0, 0, 0
    lastWasSame = lastWasCopy = False
    blockStart = 0
    for i, symbol in enumerate(data):
        if symbol == e.R:
            if not lastWasSame:
                if rleChangeCount >= 10:
                    e.copy(blockStart, copyCount - rleChangeCount)
                    blockStart += copyCount
                    e.change(i - rleChangeCount, rleChangeCount, lastSymbol)
                    copyCount, rleSymbolCopyCount, rleCount, lastWasSame, rleChangeCount = 1, 0, 0, False, 1
                else:
                    rleCount = 1
                    rleSymbolCopyCount += 1
                    lastWasSame = True
                    rleChangeCount = 0
                lastSymbol = symbol
            else:
                rleCount += 1
                rleSymbolCopyCount += 1
                if rleCount > 14:
                    e.block(blockStart, copyCount, rleSymbolCopyCount - rleCount)
                    blockStart += copyCount
                    copyCount, rleSymbolCopyCount, lastWasSame, lastWasCopy, lastSymbol = 0, 0, True, False, symbol
        else:
            if lastWasSame and lastWasCopy:
                lastWasSame = False
                copyCount += rleCount
                rleCount = 0
            if symbol == lastSymbol:
                rleChangeCount += 1
            else:
                if rleChangeCount >= 10:
                    e.block(blockStart, copyCount - rleChangeCount, rleSymbolCopyCount)
                    blockStart += copyCount
                    copyCount, rleSymbolCopyCount = 0, 0
                    e.change(i - rleChangeCount, rleChangeCount, lastSymbol)
                rleChangeCount = 1
                lastSymbol = symbol
            if not lastWasCopy:
                e.fill(i - rleCount, rleCount)
                blockStart = i
                copyCount, rleCount, rleSymbolCopyCount, lastWasSame, lastWasCopy = 1, 0, 0, False, True
            else:
                copyCount += 1
    if lastWasCopy:
        if lastWasSame:
            copyCount += rleCount
        e.copy(blockStart, copyCount)
    else:
        e.fill(len(data) - rleCount, rleCount)
    return e.finish(), e.items


# ---- the encoder as a loop over maximal runs of equal bytes ----

def runs_of(data):
    out, i, n = [], 0, len(data)
    while i < n:
        j = i + 1
        while j < n and data[j] == data[i]:
            j += 1
        out.append((i, data[i], j - i))
        i = j
    return out


def model_compress(data):
    """The same stream decided run by run.  Every decision (FILL, change of R, raw COPY, plain or encoded symbol stretch) depends on R, the run
    lengths, the counters and the two flags; second / third / lastOccurred only choose the bits inside a symbol stretch.
      pend       length of an R-run that has not been emitted: part of the open block (inCopy) or a FILL to come
      change     length of the last run if it was not of R (a run of 10 and more makes its symbol the new R when the next run begins)
      rInBlock   bytes of R in the open block (the 7 : 2 rule)"""
    data = bytes(data)
    assert data
    e = _Enc(data)
    block, count, rInBlock, pend, change, prev = 0, 0, 0, 0, 0, 0
    inCopy = False
    for pos, v, length in runs_of(data):
        if v == e.R and change >= 10:
            # the run before this one becomes R; this run is then a run of another symbol and opens the next block
            e.copy(block, count - change)
            e.change(pos - change, change, prev)
            block, count, rInBlock, pend, change = pos, length, 0, 0, length
        elif v == e.R:
            rInBlock += length
            pend = length
            change = 0
            if length > 14:
                e.block(block, count, rInBlock - length)
                block, count, rInBlock, inCopy = pos, 0, 0, False
        else:
            if pend and inCopy:
                count += pend
                pend = 0
            if change >= 10:
                e.block(block, count - change, rInBlock)
                e.change(pos - change, change, prev)
                block, count, rInBlock = pos, 0, 0
            if not inCopy:
                e.fill(pos - pend, pend)
                block, count, rInBlock, pend, inCopy = pos, 0, 0, 0, True
            count += length
            change = length
        prev = v
    if inCopy:
        e.copy(block, count + pend)
    else:
        e.fill(len(data) - pend, pend)
    return e.finish(), e.items


def model_compress_words(data):
    """model_compress with the decision kernel's SHORTCUT (csrc/hsrle_rle8sh.hip.h: k_she_decide), restated: windows of 1 024 bytes, words of 64;
    once a block is open, nothing pends, the run before was short and R is still the R of the window's start, the whole runs from a run start to
    the word's last start are taken at once if none holds a byte of that R and none is 10 bytes long.  Same stream, same items."""
    data = bytes(data)
    n = len(data)
    e = _Enc(data)
    st = {"block": 0, "count": 0, "rIn": 0, "pend": 0, "change": 0, "prev": 0, "inCopy": False}

    def run(pos, v, length):
        if v == e.R and st["change"] >= 10:
            e.copy(st["block"], st["count"] - st["change"])
            e.change(pos - st["change"], st["change"], st["prev"])
            st.update(block=pos, count=length, rIn=0, pend=0, change=length)
        elif v == e.R:
            st["rIn"] += length
            st.update(pend=length, change=0)
            if length > 14:
                e.block(st["block"], st["count"], st["rIn"] - length)
                st.update(block=pos, count=0, rIn=0, inCopy=False)
        else:
            if st["pend"] and st["inCopy"]:
                st["count"] += st["pend"]
                st["pend"] = 0
            if st["change"] >= 10:
                e.block(st["block"], st["count"] - st["change"], st["rIn"])
                e.change(pos - st["change"], st["change"], st["prev"])
                st.update(block=pos, count=0, rIn=0)
            if not st["inCopy"]:
                e.fill(pos - st["pend"], st["pend"])
                st.update(block=pos, count=0, rIn=0, pend=0, inCopy=True)
            st["count"] += length
            st["change"] = length
        st["prev"] = v

    run_start, shortcuts = 0, 0
    for base in range(0, n, 1024):
        R0 = e.R
        for w in range(base, min(base + 1024, n), 64):
            hi = min(w + 64, n)
            starts = [p for p in range(w, hi) if p == 0 or data[p] != data[p - 1]]
            k = 0
            while k < len(starts):
                pos = starts[k]
                if pos:
                    run(run_start, data[run_start], pos - run_start)
                run_start = pos
                k += 1
                if k < len(starts) and e.R == R0 and st["inCopy"] and st["pend"] == 0 and st["change"] < 10:
                    last = starts[-1]
                    inside = starts[k - 1 :]
                    if R0 not in data[pos:last] and all(b - a < 10 for a, b in zip(inside, inside[1:])):
                        st["count"] += last - pos
                        st["change"] = last - inside[-2]
                        st["prev"] = data[inside[-2]]
                        run_start = last
                        k = len(starts)
                        shortcuts += 1
    run(run_start, data[run_start], n - run_start)
    if st["inCopy"]:
        e.copy(st["block"], st["count"] + st["pend"])
    else:
        e.fill(n - st["pend"], st["pend"])
    return e.finish(), e.items, shortcuts


# ---- the compiled reference ----

class Rle8ShReference:
    @staticmethod
    def available():
        return os.path.exists(REF_LIB)

    def __init__(self):
        self.lib = ctypes.CDLL(REF_LIB)
        for nm in ("rle8_sh_compress", "rle8_sh_decompress"):
            f = getattr(self.lib, nm)
            f.restype = ctypes.c_uint32
            f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
        self.lib.rle8_sh_bounds.restype = ctypes.c_uint32
        self.lib.rle8_sh_bounds.argtypes = [ctypes.c_uint32]

    def bounds(self, n):
        return self.lib.rle8_sh_bounds(n)

    def compress(self, data):
        """The reference's stream.  (Its bound is not one: the buffer is far larger, so body and bits never meet.)"""
        data = bytes(data)
        cap = 2 * len(data) + 256
        dst = ctypes.create_string_buffer(cap)
        n = self.lib.rle8_sh_compress(data, len(data), dst, cap)
        return dst.raw[:n]

    def decompress(self, stream, out_size):
        stream = bytes(stream)
        src = ctypes.create_string_buffer(bytes(64) + stream + bytes(64), len(stream) + 128)
        dst = ctypes.create_string_buffer(out_size + 256)
        n = self.lib.rle8_sh_decompress(ctypes.addressof(src) + 64, len(stream), dst, out_size)
        return n, dst.raw[:n]


# ---- inputs: the smallest shapes at which each rule of the encoder can go wrong ----

def geometric_runs(n, alphabet, seed, mean=6):
    rng = random.Random(seed * 7919 + alphabet * 131 + n)
    syms = [0x7F, 0x80, 0x7E, 0x00, 0xFF, 0x41, 0x42, 0x43][:alphabet] if alphabet <= 8 else list(range(alphabet))
    out = bytearray()
    while len(out) < n:
        k = 1
        while rng.random() > 1.0 / mean:
            k += 1
        out += bytes([rng.choice(syms)]) * k
    return bytes(out[:n])


def noise(n, seed, avoid=()):
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        b = rng.randrange(256)
        if b not in avoid and (not out or out[-1] != b):
            out.append(b)
    return bytes(out)


def r_rich(n, r_every, seed, R=0x7F):
    """n symbols, one in `r_every` NOT the run symbol: a block for the `7 : 2` rule."""
    rng = random.Random(seed)
    return bytes(rng.choice((1, 2, 3, 200)) if i % r_every == r_every - 1 else R for i in range(n))


def input_set():
    rng = random.Random(5)
    c = {}
    for n in (1, 2, 6, 7, 8, 13, 14, 15, 16):
        c[f"random_{n}"] = rng.randbytes(n)
        c[f"r_run_{n}"] = b"\x7F" * n
        c[f"other_run_{n}"] = b"\x11" * n
    for a in (1, 2, 3, 4, 8, 256):
        for n in (97, 1000, 3000):
            c[f"alphabet{a}_{n}"] = geometric_runs(n, a, 3)
    for first in (0x7F, 0x80, 0x7E):
        c[f"begins_with_{first:02x}"] = bytes([first]) + noise(40, first) + bytes([first]) * 3 + noise(9, first + 1)
    for k in (13, 14, 15, 16, 269, 270):
        c[f"r_run_of_{k}"] = noise(9, k) + b"\x7F" * k + noise(11, k + 1) + b"\x7F" * k
    for k in (9, 10, 11, 13, 14, 15):
        c[f"change_{k}_then_r"] = noise(5, k) + b"\x33" * k + b"\x7F" * 3 + noise(8, k) + b"\x33" * 20 + b"\x7F" * 2
        c[f"change_{k}_then_third"] = noise(5, k) + b"\x33" * k + b"\x44" * 2 + noise(8, k) + b"\x33" * 20 + b"\x55"
    for k in (6, 7, 8, 262, 263):
        c[f"raw_{k}"] = b"\x7F" * 20 + noise(k, k, avoid=(0x7F,)) + b"\x7F" * 20 + noise(3, 1, avoid=(0x7F,))
    for k in (161, 162, 416, 417, 418, 900):
        for every, side in ((4, "encoded"), (5, "encoded_edge"), (3, "plain_edge"), (2, "plain")):
            c[f"r_rich_{k}_{side}"] = noise(3, k, avoid=(0x7F,)) + r_rich(k, every, k)[: k - 3] + b"\x7F" * 20 + b"\x09"
    for times in (2, 3):
        c[f"same_symbol_{times}_times_r_between"] = b"\x05" + (b"\x21" + b"\x7F" * 3) * times + b"\x21\x22\x21"
        c[f"same_symbol_{times}_times_raw_between"] = b"\x7F" * 16 + (b"\x21" + b"\x7F" * 15 + noise(9, times, avoid=(0x7F, 0x21)) + b"\x7F" * 15) * times + b"\x21\x21"
    c["ends_inside_r_run"] = noise(30, 1) + b"\x7F" * 40
    c["ends_inside_copy"] = b"\x7F" * 40 + noise(30, 2)
    c["ends_on_pending_short_r_run"] = b"\x7F" * 40 + noise(30, 3, avoid=(0x7F,)) + b"\x7F" * 5
    c["random_3000"] = rng.randbytes(3000)
    return c


def short_coded_stretches(n):
    """Built to maximise the bits of short symbol stretches: blocks of 6 bytes (under the raw COPY's 7) between FILLs of 15."""
    out = bytearray()
    k = 0
    while len(out) < n:
        out += bytes(((k * 7 + j * 37) % 120) + 130 for j in range(6)) + b"\x7F" * 15
        k += 1
    return bytes(out[:n])


# ---- streams from the grammar: legal ones no encoder writes, and one malformed stream per refusal rule ----

def wrapped(count):
    """The stored u32 of a FILL large of `count` bytes."""
    return (count - 14) & 0xFFFFFFFF


def grammar_streams():
    """name -> stream; the expected output is the model decoder's."""
    Z, S, T, END = ("Z",), ("S",), ("T",), ("END",)
    L = lambda v: ("L", v)  # noqa: E731
    raw = noise(300, 77)
    enc161 = [Z, L(0x11), S, T, L(0x11), T, S] * 23
    enc416 = ([Z] * 9 + [L(0x42), T, T, S, L(0x42), L(0x43), Z]) * 26
    out = {
        # L S then a literal equal to lastOccurred: it PROMOTES behind an S (no encoder writes this); the T behind it shows the new list
        "literal_behind_S_promotes": [L(0x21), L(0x21), L(0x30), S, L(0x21), T, S, Z, L(0x30), T, END],
        "literal_behind_T_promotes": [L(0x21), L(0x21), L(0x30), L(0x30), T, L(0x21), T, S, Z, END],
        "three_equal_literals": [L(0x55), L(0x55), L(0x55), S, T, Z, L(0x66), S, T, END],
        "literal_equals_second_third_last": [L(0x80), T, L(0x7E), S, L(0x7E), S, T, L(0x7F), Z, END],
        "gap_between_body_and_bits": [Z, L(0x01), ("FILL", 14), ("COPY", raw[:7]), S, T, END],
        "fill_large_changes_r": [Z, ("FILLL", wrapped(300), 0x10), Z, Z, L(0x7F), ("FILL", 15), ("FILLL", wrapped(14), 0x7F), Z, END],
        "encoded_copies": [L(0x09), ("ENC", enc161), T, ("ENC", enc416[:416]), T, S, Z, ("ENC", enc161[:161]), END],
        "long_plain_stretch": ([Z] * 3 + [L(0x31), S, T, T, L(0x32), Z, S]) * 120 + [END],
        "raw_copies_cross_chunks": [("COPY", raw[:7]), ("COPY", raw[:262]), ("COPYL", raw[:263]), ("COPYL", raw), Z, ("COPYL", raw[:8]), END],
    }
    for c in (0, 9, 10, 13):
        out[f"fill_large_count_{c}_via_wrap"] = [L(0x05), ("FILLL", wrapped(c), 0x22), Z, S, ("FILLL", wrapped(c), 0x23), Z, END]
    lasts = {"Z": Z, "L": L(0x44), "S": S, "T": T, "FILL": ("FILL", 269), "FILLL": ("FILLL", wrapped(3), 0x99), "COPY": ("COPY", raw[:9]), "COPYL": ("COPYL", raw[:40]),
             "ENC": ("ENC", enc161[:161])}
    for k, t in lasts.items():
        out[f"last_token_{k}"] = [L(0x01), Z, t, END]
    streams = {}
    for name, tokens in out.items():
        probe = write_stream(1, tokens)
        body = sum(_out_bytes(t) for t in tokens)
        streams[name] = write_stream(body, tokens, gap=5 if name == "gap_between_body_and_bits" else 0)
        assert len(probe) == len(streams[name]) - (5 if name == "gap_between_body_and_bits" else 0)
    return streams


def _out_bytes(t):
    k = t[0]
    if k in "ZLST":
        return 1
    if k == "FILL":
        return t[1]
    if k == "FILLL":
        return (t[1] + 14) & 0xFFFFFFFF
    if k in ("COPY", "COPYL", "ENC"):
        return len(t[1])
    return 0


def tiny_items(pairs):
    """`pairs` times (one Z, a FILL large of one byte that changes R): two records per 2 output bytes."""
    tokens = []
    for i in range(pairs):
        tokens += [("Z",), ("FILLL", wrapped(1), i % 251)]
    return write_stream(2 * pairs, tokens + [("END",)])


def malformed_streams():
    """name -> (uncompressed size to ask for, stream): one per refusal rule of include/hsrle.h.  The first two are refused for the ARGUMENTS."""
    Z, END = ("Z",), ("END",)
    good = write_stream(30, [Z] * 5 + [("L", 1), ("FILL", 24), END])
    assert model_decompress(good) is not None
    body_into_bits = bytearray(write_stream(57, [("COPY", bytes(range(20))), END]))
    body_into_bits[8] = 50
    enc = bytearray(write_stream(500, [("ENC", ([Z, ("L", 3), Z] * 54)[:161])]))
    enc[8] = 255                                     # 416 symbols announced, the bits of 161
    out = {
        "header_size_is_not_the_output_size": (31, good),
        "stream_size_above_the_buffer": (30, good[:4] + struct.pack("<I", len(good) + 1) + good[8:]),
        "stream_shorter_than_13": (1, struct.pack("<II", 1, 12) + b"\x00\x00\x00\x00\x3F"),
        "body_reaches_consumed_bits": (57, bytes(body_into_bits)),
        "bits_reach_consumed_body": (1000, write_stream(1000, [("L", 0), ("L", 0), ("L", 0)])),
        "missing_terminator": (40, write_stream(40, [("FILL", 40)])),
        "token_passes_the_size": (10, write_stream(10, [Z, ("FILL", 20), END])),
        "copy_passes_the_size": (10, write_stream(10, [Z, ("COPY", bytes(12)), END])),
        "huge_copy_count": (10, write_stream(10, [Z, END])[:8] + struct.pack("<I", 0xFFFFFFF0) + write_stream(10, [Z, END])[12:]),
        "symbol_behind_the_last_byte": (5, write_stream(5, [Z] * 6 + [END])),
        "empty_fill_behind_the_last_byte": (5, write_stream(5, [Z] * 5 + [("FILLL", wrapped(0), 7), END])),
        "terminator_with_output_missing": (6, write_stream(6, [Z] * 5 + [END])),
        "encoded_copy_runs_out_of_bits": (500, bytes(enc)),
    }
    return good, out


def marginal_encoded_spans(groups):
    """Built to grow the most per byte: ONE span that the 7 : 2 rule admits by a single byte -- `groups` times two bytes of R and seven literals
    that never repeat and are none of R, second, third (7 * 2 r > 2 * 7 r fails by equality, three more bytes of R tip it) -- so that every block
    of 416 pays its 7 bits + 1 byte for symbols that save nothing."""
    lit = [b for b in range(1, 256) if b not in (0x7F, 0x80, 0x7E)]
    out, k = bytearray(), 0
    for _ in range(groups):
        out += b"\x7F\x7F"
        for _ in range(7):
            out.append(lit[k % len(lit)])
            k += 1
    return bytes(out) + b"\x7F\x7F\x7F\x05\x09" + b"\x7F" * 15


def raw_blocks_between_changes(n):
    """Built to grow: raw COPY large blocks of 263 bytes (no byte twice in a row, none of them R at its time) between runs of 10 that change R --
    the worst a block with its event does (include/hsrle.h: 0.75 bytes per 273)."""
    out = bytearray()
    k = 0
    while len(out) < n:
        run = 0x20 + k % 7
        out += bytes(0x40 + (j * 5 + k) % 97 for j in range(263)) + bytes([run]) * 10
        k += 1
    return bytes(out[:n])
