"""Block streams written from the packet GRAMMAR (the Short family: csrc/hsrle_parse.hip.h and Traits), not by an encoder (a helper
module like decoder_fixtures.py, not a conftest).

Every stream the GPU decoders are handed elsewhere was written by an encoder, so it holds only the forms an encoder chooses: the narrowest field
that holds a value, a symbol only where it changed, a list reference wherever the symbol is listed, runs above the emit thresholds and one terminator
form of each kind.  The decoders' contract is the reference DECODER's: every field width that can hold a value, symbols sent again, pushes of listed
symbols, the smallest counts, every terminator form.  This module writes such streams and reads them back.

  grammar(codec, mode)          what a stream of the codec looks like (family name, field rules, run length of a count)
  write(g, packets, term)       -> (stream, intended output, header offsets); tracks the Packed symbol / the move-to-front list itself
  parse(g, stream)              -> (output, Counter of named forms, [(offset, length) of every packet header])
  block(...), KINDS, LAYOUTS    4 KiB blocks of the kinds W N X T Z O below and two mixtures per wave of 64 blocks
  fixture(codec, layout, ...)   a decoder_fixtures.Fixture of such blocks (container by hsrle_testlib.build_container)
  mono(codec, size, ...)        one stream of the same kinds back to back

Block kinds:
  W  every packet in its longest form (widest count, widest range, symbol carried / pushed), smallest legal count, 0 - 3 literal bytes between: headers
     start at every offset.  Where the smallest count is a zero-length run (always behind >= 1 literal here), every other packet has a run of one symbol
  N  smallest legal counts in the narrow forms: one-symbol runs and, where the grammar has them, zero-length runs behind >= 1 literal in turn with them
  X  per field a random width among the legal ones, a random legal list operation, random re-sends, literal gaps 0 - 40 and a few of 300
  T  as X, the terminator form cycling block by block through every form of the family
  Z  one run of the whole block in the widest form
  O  the oracle's own stream of video-shaped data: the canonical control
Layouts per wave of 64 blocks (LAYOUTS), shuffled with a seed per codec: sparse, mostly Z with one or two of each other kind (ratio <= 0.18), and dense, mostly
W / N / X / T (ratio >= 0.40) -- decoder_fixtures.expected_ring's two sides, so the 64-byte and the 128-byte stream ring both run.
Packets that produce no byte (no literal, a zero-length run) are legal for the reference and REFUSED by the GPU decoders (include/hsrle.h): no kind holds one,
empty_packet_stream() builds the stream that does.
Form names (the Counter's keys) -- per packet: cnt.<w> / rng.<w> with w in d (the narrow field: u8, 7 bit, in the header word) u16 u32, and
cnt.<w>.small / rng.<w>.small where a narrower field could hold the value; cnt.min (the smallest legal count); run.zero (a zero-length run behind
literals); packet.empty (no literal, no run); hdr.longest; Packed: sym.same sym.sent sym.resent; lists: op.keep op.mtf op.push op.push.listed
op.ref.dup (a reference into a list that holds one symbol twice); Short: form.1 form.3 form.3.small.  Terminators: term.end, term.lit.<w>,
term.lit.zero (a literal terminator without literals); LUT / Short: term.c<w>.end, term.c<w>.r<w>.
"""
import collections
import random
import struct

import numpy as np

import decoder_fixtures as F
from hsrle_testlib import (CODECS, GREEDY1, GREEDY3, GREEDY7, LUT3, LUT7, PACKED, PACKED_SINGLE, PLAIN, SHORT0, SHORT1, SHORT3, SHORT7, SINGLE, SINGLE_SHORT,
                           SYNTH_VIDEO)

LUT_INIT = (0x00, 0x7F, 0xFF, 0x01, 0x7E, 0x80, 0xFE)
WIDTH_BYTES = {"d": 0, "u16": 2, "u32": 4}

Packet = collections.namedtuple("Packet", "lit sym cnt cw rw carry op short3", defaults=(False, None, False))
Term = collections.namedtuple("Term", "end lit cw rw", defaults=(b"", "u16", "u32"))


class Grammar:
    """The field rules of one codec's streams.  kind: 'plain' (sym, cnt:u8|0+u32, range:u8|0+u32), 'packed' (same/cnt byte, symbol if not same, range
    7-bit-or-u32 or the plain one), 'single' (the plain fields without a symbol), 'lut' (u16 word, symbol, extensions), 'short' (1 or 3 byte word,
    extensions, symbol)."""

    def __init__(self, codec, mode=None):
        fam, S, al = codec.family, codec.S, bool(codec.aligned) and codec.S > 1
        self.codec, self.S, self.aligned = codec, S, al
        self.mode = None                    # the 9th header byte of the 8 bit plain / Packed / Single streams
        self.stream_symbol = False          # one symbol byte behind the header, none in the packets
        self.K, self.range7, self.min_cnt = 0, False, 1
        if fam in (SINGLE, PACKED_SINGLE):
            self.mode = 1 if mode is None else mode
            if self.mode == 0:
                fam = PLAIN if fam == SINGLE else PACKED
        elif fam in (PLAIN, PACKED) and S == 1:
            self.mode = 0
        if fam in (SINGLE, PACKED_SINGLE):
            self.kind, self.family, self.stream_symbol = "single", "single", True
            self.short = 4 if fam == SINGLE else 2
        elif fam == PLAIN:
            self.kind, self.family, self.short = "plain", "plain", (6 if S == 1 else S + 4)
        elif fam == PACKED:
            self.kind, self.range7, self.short = "packed", not al, 3
            self.family = "packed7" if self.range7 else "packed_sym"
        elif fam in (LUT3, LUT7):
            self.kind, self.K, self.min_cnt = "lut", (3 if fam == LUT3 else 7), 2
            self.family, self.RB = f"lut{self.K}", (7 if fam == LUT3 else 6)
        else:
            self.kind, self.min_cnt = "short", 2
            self.K = {SHORT0: 0, SHORT1: 1, SHORT3: 3, SHORT7: 7, GREEDY1: 1, GREEDY3: 3, GREEDY7: 7, SINGLE_SHORT: 0}[fam]
            self.stream_symbol = fam == SINGLE_SHORT
            self.family = "single_short" if self.stream_symbol else f"short{self.K}"
            # the header byte: [list index SLB | count SCB | range SRBP]; the 3-byte form: a 9 bit count (7-symbol list: 10 bits, values to 511) and SRB range bits
            self.SLB = {0: 0, 1: 1, 3: 2, 7: 3}[self.K]
            self.SCB = {0: 4, 1: 3, 3: 3, 7: 2}[self.K]
            self.SRBP = 8 - self.SLB - self.SCB
            self.SRB = 24 - self.SLB - (self.SRBP if self.K == 7 else self.SCB) - 9
            self.SCINV = (1 << self.SCB) - 1
            self.mins = 2 if (self.K or self.stream_symbol) else S + 2
        if S == 16:
            self.family = "w128"
        self.header = 9 if self.mode is not None else 8
        self.listed = self.kind in ("lut", "short") and self.K > 0
        self.carries = not self.stream_symbol                     # packets can carry a symbol

    # ---- values
    def run_bytes(self, cnt):
        S = self.S
        if self.kind == "lut":
            return (cnt + 3 // S - 2) * S if self.aligned else cnt + 1
        if self.kind == "short":
            return (cnt + self.mins // S - 2) * S if self.aligned else cnt + self.mins - 2
        return (cnt + self.short // S - 1) * S if self.aligned else cnt + self.short - 1

    def cnt_for(self, n):
        """The largest count whose run has at most n bytes."""
        a = self.run_bytes(3) - self.run_bytes(2)
        return (n - (self.run_bytes(2) - 2 * a)) // a

    def first_run_cnt(self):
        """The smallest count with a run of at least one byte."""
        c = self.min_cnt
        while self.run_bytes(c) == 0:
            c += 1
        return c

    @property
    def has_empty(self):
        return self.run_bytes(self.min_cnt) == 0

    @property
    def bias(self):
        """range = literals + bias"""
        return 2 if self.kind in ("lut", "short") else 1

    def initial_list(self):
        if self.kind == "packed":
            return [bytes(self.S)]
        return [bytes([v]) * self.S for v in LUT_INIT[: self.K]] if self.listed else []

    # ---- widths a field value may take
    def cnt_widths(self, v):
        if self.kind in ("plain", "single"):
            return (["d"] if 1 <= v <= 255 else []) + ["u32"]
        if self.kind == "packed":
            return (["d"] if 1 <= v <= 127 else []) + ["u32"]
        top = 127 if self.kind == "lut" else 511
        return (["d"] if 2 <= v <= top else []) + (["u16"] if 1 <= v <= 0xFFFF else []) + ["u32"]

    def rng_widths(self, v):
        if self.kind in ("plain", "single") or (self.kind == "packed" and not self.range7):
            return (["d"] if 1 <= v <= 255 else []) + ["u32"]
        if self.kind == "packed":
            return (["d"] if 1 <= v <= 127 else []) + ["u32"]
        top = (1 << self.RB) - 1 if self.kind == "lut" else (1 << self.SRB) - 1
        return (["d"] if 2 <= v <= top else []) + (["u16"] if 1 <= v <= 0xFFFF else []) + ["u32"]

    def fits_short1(self, cnt, rng):
        return self.kind == "short" and 2 <= cnt <= self.SCINV + 1 and 2 <= rng <= (1 << self.SRBP) + 1


def grammar(codec, mode=None):
    return Grammar(codec, mode)


def _fill(sym, n):
    return (sym * (n // len(sym) + 1))[:n]


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# writer


class Writer:
    def __init__(self, g, symbol=None):
        self.g, self.s, self.out, self.headers = g, bytearray(g.header), bytearray(), []
        if g.mode is not None:
            self.s[8] = g.mode
        self.symbol = None
        if g.stream_symbol:
            self.symbol = bytes(symbol) if symbol is not None else b"\x00"
            self.s += self.symbol
        self.state = g.initial_list()

    def _ext(self, w, v):
        return b"" if w == "d" else struct.pack("<H" if w == "u16" else "<I", v)

    def _op(self, sym, op):
        """the list operation: (index written, carries the symbol)"""
        g, st = self.g, self.state
        if op is None:
            op = st.index(sym) if sym in st else g.K
        if op == g.K:
            self.state = [sym] + st[:-1]
            return op, True
        assert st[op] == sym, "a list reference must name the packet's symbol"
        st.insert(0, st.pop(op))
        return op, False

    def _word(self, idx, cnt, rng, cw, rw, short3, sym):
        """Short: the 1 or 3 byte word, the extensions, then the symbol.  LUT: the u16 word, the symbol, the extensions."""
        g = self.g
        cf = cnt if cw == "d" else (1 if cw == "u16" else 0)
        rf = rng if rw == "d" else (1 if rw == "u16" else 0)
        if g.kind == "lut":
            return struct.pack("<H", (idx << (14 if g.K == 3 else 13)) | (cf << g.RB) | rf) + sym + self._ext(cw, cnt) + self._ext(rw, rng)
        if cw == "d" and rw == "d" and not short3 and g.fits_short1(cnt, rng):
            return bytes([(idx << (g.SCB + g.SRBP)) | ((cnt - 2) << g.SRBP) | (rng - 2)]) + sym
        assert cf <= 511 and rf < (1 << g.SRB)
        v = (idx << (g.SCB + g.SRBP + 16)) | (g.SCINV << (g.SRBP + 16)) | (cf << g.SRB) | rf
        return bytes([v >> 16, (v >> 8) & 0xFF, v & 0xFF]) + self._ext(cw, cnt) + self._ext(rw, rng) + sym

    def _plain_fields(self, cnt, cw, rng, rw, head, sym):
        """plain / Packed / Single: [same | ] count, symbol (Packed: behind the count), range"""
        g = self.g
        c = bytes([head | (cnt if cw == "d" else 0)]) + (b"" if cw == "d" else struct.pack("<I", cnt))
        if g.range7:
            r = bytes([rng << 1]) if rw == "d" else struct.pack("<I", (rng << 1) | 1)
        else:
            r = bytes([rng]) if rw == "d" else b"\x00" + struct.pack("<I", rng)
        return (c + sym + r) if g.kind == "packed" else (sym + c + r)

    def packet(self, p):
        g = self.g
        sym = self.symbol if g.stream_symbol else bytes(p.sym)
        assert len(sym) == g.S and p.cnt >= g.min_cnt
        rng = len(p.lit) + g.bias
        assert p.cw in g.cnt_widths(p.cnt) and p.rw in g.rng_widths(rng), (p.cnt, p.cw, rng, p.rw)
        self.headers.append(len(self.s))
        if g.kind in ("lut", "short"):
            idx, carried = self._op(sym, p.op) if g.listed else (0, g.carries)
            self.s += self._word(idx, p.cnt, rng, p.cw, p.rw, p.short3, sym if carried else b"")
        elif g.kind == "packed":
            same = sym == self.state[0] and not p.carry
            self.state[0] = sym
            self.s += self._plain_fields(p.cnt, p.cw, rng, p.rw, 0x80 if same else 0, b"" if same else sym)
        else:
            self.s += self._plain_fields(p.cnt, p.cw, rng, p.rw, 0, sym if g.carries else b"")
        self.headers[-1] = (self.headers[-1], len(self.s) - self.headers[-1])
        self.s += p.lit
        self.out += p.lit + _fill(sym, g.run_bytes(p.cnt))

    def finish(self, t):
        g, n = self.g, len(t.lit)
        assert not (t.end and n)
        self.headers.append(len(self.s))
        if g.kind in ("lut", "short"):
            rng, rw = (0, "u16") if t.end else (n + 2, t.rw)
            assert t.cw in ("u16", "u32") and rw in g.rng_widths(max(rng, 1))
            sym = b"" if (g.K or g.stream_symbol) else (b"\x00" if t.end else bytes(g.S))    # no list: the end terminator carries ONE zero byte
            self.s += self._word(0, 0, rng, t.cw, rw, True, sym)
        else:
            rng, rw = (0, "u32") if t.end else (n + 1, t.rw)
            assert rw in g.rng_widths(max(rng, 1))
            packed = g.kind == "packed"
            self.s += self._plain_fields(0, "u32", rng, rw, 0x80 if packed else 0, b"" if (packed or not g.carries) else bytes(g.S))
        self.headers[-1] = (self.headers[-1], len(self.s) - self.headers[-1])
        self.s += t.lit
        self.out += t.lit
        struct.pack_into("<II", self.s, 0, len(self.out), len(self.s))
        return bytes(self.s), bytes(self.out), self.headers


def write(g, packets, term, symbol=None):
    """(stream, intended output, [(offset, length) of every header, the terminator's last])"""
    w = Writer(g, symbol)
    for p in packets:
        w.packet(p)
    return w.finish(term)


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# parser


def parse(g, stream):
    """(output, Counter of form names, [(offset, length) of every header]) of a stream of grammar g; AssertionError if it is not one."""
    s = bytes(stream)
    U, C = struct.unpack_from("<II", s, 0)
    assert C == len(s), "the header's compressed size is the stream's"
    if g.mode is not None:
        assert s[8] == g.mode, "mode byte"
    p = g.header
    forms, out, headers = collections.Counter(), bytearray(), []
    symbol = None
    if g.stream_symbol:
        symbol, p = s[p : p + 1], p + 1
    state = g.initial_list()

    def take(n):
        nonlocal p
        assert p + n <= C, "a field behind the end of the stream"
        p += n
        return s[p - n : p]

    def ext(w):
        return 0 if w == "d" else int.from_bytes(take(WIDTH_BYTES[w]), "little")

    def list_op(idx):
        assert idx <= g.K
        dup = len(set(state)) < len(state)
        if idx == g.K:
            sym = take(g.S)
            forms["op.push"] += 1
            forms["op.push.listed"] += sym in state
            state[:] = [sym] + state[:-1]
        else:
            forms["op.keep" if idx == 0 else "op.mtf"] += 1
            forms["op.ref.dup"] += dup
            state.insert(0, state.pop(idx))

    while True:
        at = p
        longest = True
        if g.kind in ("lut", "short"):
            if g.kind == "lut":
                v = int.from_bytes(take(2), "little")
                idx, cf, rf = v >> (14 if g.K == 3 else 13), (v >> g.RB) & 0x7F, v & ((1 << g.RB) - 1)
                list_op(idx)
                three = True
            else:
                b = take(1)[0]
                idx, c3 = (b >> (g.SCB + g.SRBP)) if g.K else 0, (b >> g.SRBP) & g.SCINV
                three = c3 == g.SCINV
                if three:
                    v = (b << 16) | int.from_bytes(take(2), "big")
                    cf, rf = (v >> g.SRB) & ((1 << (g.SRBP + 16 - g.SRB)) - 1), v & ((1 << g.SRB) - 1)
                else:
                    cf, rf = c3 + 2, (b & ((1 << g.SRBP) - 1)) + 2
            cw = "d" if (cf >= 2 or not three) else ("u16" if cf == 1 else "u32")
            rw = "d" if (rf >= 2 or not three) else ("u16" if rf == 1 else "u32")
            cnt = cf if cw == "d" else ext(cw)
            rng = rf if rw == "d" else ext(rw)
            end = rw == "u16" and rng == 0
            if g.kind == "short" and not end:
                if g.listed:
                    list_op(idx)
                elif g.carries:
                    state[:] = [take(g.S)]
            if g.kind == "short" and end and not g.K and g.carries:
                take(1)
            sym = symbol if g.stream_symbol else (state[0] if state else None)
            last = end or cnt == 0
            if last:
                forms[f"term.c{cw}.end" if end else f"term.c{cw}.r{rw}"] += 1
            elif g.kind == "short":
                forms["form.3" if three else "form.1"] += 1
                forms["form.3.small"] += three and cw == "d" and rw == "d" and g.fits_short1(cnt, rng)
            assert end or rng >= 2, "a range below 2"
            longest = cw == "u32" and rw == "u32" and (not g.listed or idx == g.K)
        else:
            if g.kind == "packed":
                b = take(1)[0]
                same, cf = bool(b & 0x80), b & 0x7F
                cw = "d" if cf else "u32"
                cnt = cf if cf else ext("u32")
                if not same:
                    sym = take(g.S)
                    if cnt:
                        forms["sym.resent" if sym == state[0] else "sym.sent"] += 1
                    state[0] = sym
                elif cnt:
                    forms["sym.same"] += 1
                sym = state[0]
                longest = not same
            else:
                sym = take(g.S) if g.carries else symbol
                cf = take(1)[0]
                cw = "d" if cf else "u32"
                cnt = cf if cf else ext("u32")
            if g.range7:
                assert p < C
                rw = "u32" if s[p] & 1 else "d"
                rng = int.from_bytes(take(4 if rw == "u32" else 1), "little") >> 1
            else:
                r0 = take(1)[0]
                rw = "d" if r0 else "u32"
                rng = r0 if r0 else ext("u32")
            end = rw == "u32" and rng == 0
            last = end or cnt == 0
            if last and g.range7 and g.S == 16 and rw == "d" and rng == 0 and C - p == 4:
                # the 128 bit encoders close a stored last run with the PLAIN end terminator whatever the range field: a 7 bit range of 0, four bytes unread
                assert take(4) == bytes(4)
                forms["term.end.q11"] += 1
            elif last:
                forms["term.end" if end else f"term.lit.{rw}"] += 1
            longest = longest and cw == "u32" and rw == "u32"
        headers.append((at, p - at))
        lit = 0 if end else max(rng - g.bias, 0)
        out += take(lit)
        if last:
            forms["term.lit.zero"] += (not end) and lit == 0
            break
        run = g.run_bytes(cnt)
        forms[f"cnt.{cw}"] += 1
        forms[f"rng.{rw}"] += 1
        forms[f"cnt.{cw}.small"] += cw != g.cnt_widths(cnt)[0]
        forms[f"rng.{rw}.small"] += rw != g.rng_widths(rng)[0]
        forms["cnt.min"] += cnt == g.min_cnt
        forms["run.zero"] += run == 0 and lit > 0
        forms["packet.empty"] += run == 0 and lit == 0
        forms["hdr.longest"] += longest
        out += _fill(sym, run)
    assert p == C, f"{C - p} bytes behind the terminator"
    assert len(out) == U, f"the stream holds {len(out)} bytes, its header says {U}"
    return bytes(out), +forms, headers


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# block kinds

KINDS = "WNXTZO"
LAYOUTS = {"sparse": (("W", 1), ("N", 1), ("X", 1), ("T", 1), ("O", 2), ("Z", 58)),      # ratio <= 0.18
           "dense": (("W", 14), ("N", 12), ("X", 14), ("T", 12), ("O", 6), ("Z", 6))}    # ratio >= 0.40
WAVE = F.WAVE
RESERVE = 64              # output bytes a block's generator leaves to the closing packet and the terminator


def term_forms(g):
    """Every terminator form of the family: (end, literal count or None = what is left, count width, range width)."""
    if g.kind in ("lut", "short"):
        return [(e, n, cw, rw) for cw in ("u16", "u32") for e, n, rw in ((True, 0, "u16"), (False, None, "d"), (False, None, "u16"), (False, None, "u32"), (False, 0, "d"), (False, 0, "u32"))]
    return [(True, 0, "u32", "u32"), (False, None, "u32", "u32"), (False, None, "u32", "d"), (False, 0, "u32", "u32"), (False, 0, "u32", "d")]


def _pick_op(g, rng, state, sym, push):
    if not g.listed:
        return None
    refs = [j for j, e in enumerate(state) if e == sym]
    return g.K if (push or not refs) else rng.choice(refs)


def gen_packets(g, kind, n, rng, syms, w):
    """Packets of `kind` for about n output bytes, written to Writer w; returns the bytes they produced."""
    start = len(w.out)
    lits = rng.randbytes
    while True:
        left = n - (len(w.out) - start)
        sym = rng.choice(syms)
        if kind == "N" and g.kind == "packed" and rng.random() < 0.75:     # narrow: mostly the `same` bit
            sym = w.state[0] if w.state[0] in syms else sym
        if kind == "W":
            # (where the smallest count is a zero-length run, every other packet has a run of one symbol: the stream stays below four times its output)
            cnt = g.first_run_cnt() if (g.has_empty and len(w.headers) % 2) else g.min_cnt
            lit, cw, rw, carry, push, s3 = rng.randrange(4), "u32", "u32", True, True, True
        elif kind == "N":
            cnt = g.first_run_cnt() if (g.has_empty and len(w.headers) % 2) else g.min_cnt     # (zero-length runs and one-symbol runs in turn)
            lit, cw, rw, carry, push, s3 = rng.randrange(4), "d", "d", False, False, False
        else:
            cnt = g.min_cnt + rng.choice((0, 0, 1, 2, 3, 5, 9, 17, 40, 130, 300))
            lit = 300 if rng.random() < 0.03 else rng.randrange(41)
            cw, rw = rng.choice(g.cnt_widths(cnt)), rng.choice(g.rng_widths(lit + g.bias))
            carry, push, s3 = rng.random() < 0.3, rng.random() < 0.3, rng.random() < 0.5
            if g.kind == "short" and rng.random() < 0.15:              # the values of the one-byte form in the three-byte form
                cnt, lit, cw, rw, s3 = g.min_cnt + rng.randrange(g.SCINV), rng.randrange(4), "d", "d", True
        run = g.run_bytes(cnt)
        lit = max(lit, 1) if run == 0 else lit
        if run + lit > left:
            if g.run_bytes(g.first_run_cnt()) + 44 > left:
                return len(w.out) - start
            continue
        if kind not in "WN":
            rw = rw if rw in g.rng_widths(lit + g.bias) else "u32"
        w.packet(Packet(lits(lit), sym, cnt, cw, rw, carry, _pick_op(g, rng, w.state, sym, push), s3))


def close(g, w, left, rng, syms, form, wide):
    """The last packets and the terminator: exactly `left` more output bytes.  form: a term_forms() entry."""
    end, n, cw, rw = form
    lits = rng.randbytes
    if n is None:
        n = min(left, _narrow_cap(g, rw))
    if left > n:
        cnt = g.first_run_cnt()
        run = g.run_bytes(cnt)
        k = left - n - run
        if k < 0:
            n, k = left - run, 0
            assert n >= 0
        sym = rng.choice(syms)
        wd = "u32" if wide else None
        w.packet(Packet(lits(k), sym, cnt, wd or g.cnt_widths(cnt)[0], wd or g.rng_widths(k + g.bias)[0], wide, _pick_op(g, rng, w.state, sym, wide), wide))
    if rw not in g.rng_widths(n + g.bias):
        rw = "u32"
    return w.finish(Term(end, lits(0 if end else n), cw, "u16" if (end and g.kind in ("lut", "short")) else rw))


def _narrow_cap(g, rw):
    """the most literals a terminator's range field of width rw holds"""
    if rw != "d":
        return (0xFFFF if rw == "u16" else 1 << 30) - g.bias
    if g.kind == "lut":
        return (1 << g.RB) - 1 - g.bias
    if g.kind == "short":
        return (1 << g.SRB) - 1 - g.bias
    return (127 if g.range7 else 255) - g.bias


def block(codec, kind, n, rng, term_index=0, video=None, mode=None):
    """(stream, output) of one block of n output bytes."""
    g = grammar(codec, mode)
    if kind == "O":
        assert video is not None and len(video) == n and mode is None
        return F.oracle_instance().compress(codec, bytes(video)), bytes(video)
    syms = F._symbols(rng, g.S)
    w = Writer(g, syms[0] if g.stream_symbol else None)
    forms = term_forms(g)
    if kind == "Z":
        cnt = g.cnt_for(n)
        sym = syms[0]
        w.packet(Packet(b"", sym, cnt, "u32", "u32", True, g.K if g.listed else None, True))
        left = n - g.run_bytes(cnt)
        return w.finish(Term(left == 0, rng.randbytes(left), "u32", "u32"))[:2]
    done = gen_packets(g, "X" if kind == "T" else kind, n - RESERVE, rng, syms, w)
    form = forms[term_index % len(forms)] if kind == "T" else (forms[1] if kind == "W" else (forms[2] if kind == "N" else rng.choice(forms)))
    if kind == "W" and g.kind in ("lut", "short"):
        form = (False, None, "u32", "u32")
    return close(g, w, n - done, rng, syms, form, kind == "W")[:2]


def wave_kinds(layout, rng):
    kinds = [k for k, c in LAYOUTS[layout] for _ in range(c)]
    assert len(kinds) == WAVE
    rng.shuffle(kinds)
    return kinds


_CACHE = collections.OrderedDict()


def fixture(codec, layout, B=4096, blocks=None, last_len=None, modes=(None,)):
    """A decoder_fixtures.Fixture of grammar blocks: three waves of B-byte blocks by default, the last block partial and off a 16-byte boundary.
    modes: the Single ids take modes[i % len(modes)] for block i (mode 0: the multi-symbol grammar under the Single id).  fix.data is the INTENDED output."""
    key = (codec.key, layout, B, blocks, last_len, modes)
    if key in _CACHE:
        _CACHE.move_to_end(key)
        return _CACHE[key]
    if blocks is None:
        blocks, dflt = F.default_shape(B)
        last_len = dflt if last_len is None else last_len
    rng = random.Random(7919 * CODECS.index(codec) + 13 * B + (5 if layout == "dense" else 0) + 3)
    kinds = []
    while len(kinds) < blocks:
        kinds += wave_kinds(layout, rng)
    kinds = kinds[:blocks]
    video = F.oracle_instance().synth(SYNTH_VIDEO, codec.S, 23 + CODECS.index(codec), blocks * B)
    streams, outs, t = [], [], 0
    for i, kind in enumerate(kinds):
        n = last_len if i == blocks - 1 else B
        mode = modes[i % len(modes)]
        if kind == "O" and mode is not None:
            kind = kinds[i] = "X"
        s, o = block(codec, kind, n, rng, t, video[i * B : i * B + n], mode)
        t += kind == "T"
        assert len(o) == n
        streams.append(s)
        outs.append(o)
    fix = F.assemble(codec, layout, B, np.frombuffer(b"".join(outs), dtype=np.uint8), kinds, streams)
    _CACHE[key] = fix
    while len(_CACHE) > 12:
        _CACHE.popitem(last=False)
    return fix


# what the fixtures add to the forms the encoders write, per family (tests/test_stream_grammar.py proves it: a census of the encoder-written fixtures of
# decoder_fixtures finds none of them), and how often a codec's fixtures must hold each: packet forms / terminator forms
_WIDE = ("cnt.u32.small", "rng.u32.small", "term.lit.d")
_WIDE8 = _WIDE + ("hdr.longest", "rng.u32", "term.lit.zero")
_LIST = ("cnt.u16.small", "cnt.u32", "cnt.u32.small", "rng.u16.small", "rng.u32", "rng.u32.small", "hdr.longest", "term.cu16.rd", "term.cu16.ru16", "term.cu32.end",
         "term.cu32.rd", "term.cu32.ru16", "term.cu32.ru32", "term.lit.zero")
NEW_FORMS = {"plain": _WIDE8, "single": _WIDE8, "packed7": _WIDE8, "packed_sym": _WIDE8 + ("cnt.min", "sym.resent", "run.zero"), "w128": _WIDE + ("sym.resent", "run.zero"),
             "lut3": _LIST + ("op.push.listed", "op.ref.dup", "run.zero"), "lut7": _LIST + ("op.push.listed", "op.ref.dup", "run.zero"),
             "short0": _LIST + ("form.3.small", "rng.u16"), "single_short": _LIST + ("form.3.small", "rng.u16"),
             "short1": _LIST + ("form.3.small", "rng.u16", "op.push.listed", "run.zero"),
             "short3": _LIST + ("form.3.small", "rng.u16", "op.push.listed", "op.ref.dup", "run.zero"),
             "short7": _LIST + ("form.3.small", "rng.u16", "op.push.listed", "op.ref.dup", "run.zero")}
MIN_PACKET_FORMS, MIN_TERM_FORMS = 50, 2


def new_forms(g):
    """The forms of NEW_FORMS that the codec's grammar has: zero-length runs where the smallest count gives one, re-sent symbols where packets carry state."""
    have = {"run.zero": g.has_empty, "sym.resent": g.kind == "packed", "cnt.min": True}
    return [f for f in NEW_FORMS[g.family] if have.get(f, True)]


# forms the compiled reference refuses or decodes to other bytes: (family, form) -> reason.  None: it decodes every form written here.
EXCLUDED = {}

MONO_SIZE, MONO_LONG = 40000, 300000
MONO_LONG_CODECS = ("rle8_packed_multi", "rle8_7symlut", "rle16_sym", "rle32_byte_packed", "rle24_3symlut_byte_short", "rle64_7symlut_byte_short", "rle128_sym_packed", "rle8_single_short")


def mono(codec, size=MONO_SIZE, long_literals=False, seed=0):
    """(stream, output): sections of the kinds W N X Z back to back in ONE stream of `size` output bytes; long_literals: also stretches of several KiB of
    literals (one packet's), so that a walk from entry to entry passes whole regions without a header."""
    g = grammar(codec)
    rng = random.Random(104729 * CODECS.index(codec) + size + seed)
    syms = F._symbols(rng, g.S)
    w = Writer(g, syms[0] if g.stream_symbol else None)
    order = "WXNZXW" if not long_literals else "XLWXZLNX"
    k = 0
    while size - len(w.out) > 4096 + RESERVE:
        kind, k = order[k % len(order)], k + 1
        if kind in "ZL" and size - len(w.out) < 17000 + 4096:
            kind = "X"
        if kind == "Z":
            sym, cnt = rng.choice(syms), g.cnt_for(rng.choice((3000, 9000)))
            w.packet(Packet(b"", sym, cnt, "u32", "u32", True, _pick_op(g, rng, w.state, sym, True), True))
        elif kind == "L":
            sym, cnt, n = rng.choice(syms), g.first_run_cnt(), rng.choice((5000, 9001, 17000))
            lit = np.random.RandomState(rng.randrange(1 << 31)).randint(0, 256, n, dtype=np.uint8).tobytes()
            w.packet(Packet(lit, sym, cnt, g.cnt_widths(cnt)[-1], "u32", False, _pick_op(g, rng, w.state, sym, False), True))
        else:
            gen_packets(g, kind, min(rng.choice((1500, 4000)), size - len(w.out) - RESERVE), rng, syms, w)
    return close(g, w, size - len(w.out), rng, syms, rng.choice(term_forms(g)), False)[:2]


def empty_packet_stream(codec, n=4096, seed=0):
    """(stream, output) of a block of n bytes of kind N with packets that produce no byte (no literal, a zero-length run) among them -- only for grammars that
    have such packets (g.has_empty)."""
    g = grammar(codec)
    assert g.has_empty
    rng = random.Random(31337 * CODECS.index(codec) + seed)
    syms = F._symbols(rng, g.S)
    w = Writer(g, None)
    while n - len(w.out) > 600:
        gen_packets(g, "N", 200, rng, syms, w)
        sym = rng.choice(syms)
        w.packet(Packet(b"", sym, g.min_cnt, "d", "d", False, _pick_op(g, rng, w.state, sym, False), False))
    return close(g, w, n - len(w.out), rng, syms, term_forms(g)[1], False)[:2]
