"""Containers for the order of the three sections (header, literals, run) of a trip of the 8 bit packet loop of k_decode_blocks (a helper module like
decoder_fixtures.py and stream_grammar.py, not a conftest).  Every stream is PLACED packet by packet with the writers of stream_grammar.py -- where a packet
starts and ends relative to the decoder's 128-byte steps is the point -- and the containers come from hsrle_testlib.build_container.

Blocks of B = 256 / 384 bytes (two / three steps), 64 / 65 blocks (one full wave, plus one active lane), every codec id of one-byte symbols.  Block kinds, a
step boundary being an output position 128 k inside the block:
  R1 R15 R16 R17 R127   a run that crosses a step boundary by that many bytes            (the lane enters the next step with run != 0: R alone, then a header)
  R256                  a run of >= 256 bytes: one whole step has no header for the lane
  L1 L15 L16 L17 L127   a literal stretch that crosses a step boundary by that many bytes (the lane enters with lit != 0: L, R, then a header)
  LL                    a literal stretch of more than 128 bytes: more than a 64-byte ring holds, and more than a 128-byte ring holds behind a misaligned stream
                        position -- a stall in L and a second pass that re-enters at L
  E                     a packet that ends exactly on a step boundary: the next step begins with a header (the header-only trip)
  T                     the last packet ends exactly on a step boundary AND at the block's end; behind it one terminator form without literals, cycling through
                        every such form of the grammar (last_forms) over the containers of a codec and mixture
  H                     >= 12 headers in their longest form back to back, 0 - 3 literals between: > 140 stream bytes of them, so one straddles the end of the
                        resident ring bytes wherever that lies (a header stall at the end of a trip)
  D                     a packet every few bytes: narrow headers, the smallest run, 0 - 2 literals
  I                     one run of the whole block: the neighbour that is done after one packet
Mixtures per wave of 64 blocks (MIXTURES): sparse, every kind once or twice beside idle neighbours (ratio <= 0.18: the 64-byte ring), and dense, the literal and
packet-dense kinds many times over (ratio >= 0.40: the 128-byte ring).

Malformed streams (MALFORMED) replace ONE block (VICTIM) of a container:
  cut_literal      the stream ends inside a literal stretch (its size field says so too: the header is consistent, the packet chain is not)
  cut_header_1     ... one byte into a packet header
  cut_header_mid   ... in the middle of a header in its longest form
  early_end        a terminator in the middle of the block.  The 8 bit grammars have no packet that produces nothing (every count >= 1 has a run of >= 2 bytes,
                   count 0 IS the terminator), so this is their `empty packet`: nothing left to do while bytes are still owed
  range_below_2    list and Short grammars only: a range field of 1 (fewer than zero literals) -- the other packet without a meaning
  literal_leaves   a literal count of 0x7FFFFF00: the stretch leaves the stream
  no_terminator    a T block whose terminator is cut off: every byte is produced, only the end mark is missing
What the decoders must say about each is what the PARENT of the change said (tests/golden/decode_loop_order_status.json).
"""
import collections
import random
import struct

import numpy as np

import decoder_fixtures as F
import stream_grammar as G
from hsrle_testlib import CODECS

STEP = 128
CROSS = (1, 15, 16, 17, 127)
CODECS8 = [c for c in CODECS if c.S == 1]
BLOCK_SIZES = (256, 384)
BLOCK_COUNTS = (64, 65)
SHAPES = [(B, n) for B in BLOCK_SIZES for n in BLOCK_COUNTS]
SPECIAL = tuple(f"R{x}" for x in CROSS) + ("R256",) + tuple(f"L{x}" for x in CROSS) + ("LL", "E", "T", "T", "H", "D")
MIXTURES = {"sparse": SPECIAL + ("I",) * (64 - len(SPECIAL)),
            "dense": SPECIAL + ("LL",) * 25 + ("D",) * 10 + ("H",) * 4 + ("I",) * (64 - len(SPECIAL) - 39)}
KINDS = tuple(dict.fromkeys(SPECIAL + ("I",)))
MALFORMED = ("cut_literal", "cut_header_1", "cut_header_mid", "early_end", "range_below_2", "literal_leaves", "no_terminator")
VICTIM = 5
SUB_BLOCK = 128            # the entry-record decode: one lane per 128 output bytes

Block = collections.namedtuple("Block", "kind stream out events term headers")   # events: (first literal, first run byte, end, wide header) per packet


def last_forms(g):
    """Every terminator form of the grammar that carries no literal: (end, count width, range width)."""
    if g.kind in ("lut", "short"):
        return [(e, cw, rw) for cw in ("u16", "u32") for e, rw in ((True, "u16"), (False, "d"), (False, "u16"), (False, "u32"))]
    return [(True, "u32", "u32"), (False, "u32", "u32"), (False, "u32", "d")]


def malformed_kinds(codec):
    return [m for m in MALFORMED if m != "range_below_2" or G.grammar(codec).kind in ("lut", "short")]


class _Builder:
    def __init__(self, codec, B, rng):
        self.g, self.B, self.rng = G.grammar(codec), B, rng
        self.syms = F._symbols(rng, 1)
        self.w = G.Writer(self.g, self.syms[0] if self.g.stream_symbol else None)
        self.min_run = self.g.run_bytes(self.g.min_cnt)
        self.events = []

    @property
    def o(self):
        return len(self.w.out)

    def pkt(self, lit, run, wide=False):
        g, rng = self.g, self.rng
        cnt = g.cnt_for(run)
        assert cnt >= g.min_cnt and g.run_bytes(cnt) == run, (run, cnt)
        sym = rng.choice(self.syms)
        cw = "u32" if wide else g.cnt_widths(cnt)[0]
        rw = "u32" if wide else g.rng_widths(lit + g.bias)[0]
        o = self.o
        self.w.packet(G.Packet(rng.randbytes(lit), sym, cnt, cw, rw, wide, G._pick_op(g, rng, self.w.state, sym, wide), wide))
        self.events.append((o, o + lit, o + lit + run, wide))

    def to(self, pos, lit=0):
        """one packet that ends at output position pos"""
        self.pkt(lit, pos - self.o - lit)

    def finish(self, form=None, tail=None):
        """Fill the block: a packet up to its end where there is room for one (unless tail == "literals"), else the rest as the terminator's literals; then the
        terminator."""
        g, left = self.g, self.B - self.o
        if left >= self.min_run + 2 and tail != "literals":
            self.to(self.B, lit=2)
            left = 0
        if left == 0:
            end, cw, rw = form if form is not None else last_forms(g)[0]
            term = G.Term(end, b"", cw, rw)
        else:
            assert form is None
            term = G.Term(False, self.rng.randbytes(left), "u16", g.rng_widths(left + g.bias)[0])
        stream, out, headers = self.w.finish(term)
        assert len(out) == self.B
        return stream, out, headers, term


def build_block(codec, kind, B, rng, form=None):
    b, tail = _Builder(codec, B, rng), None
    steps = B // STEP
    at = STEP * (1 + rng.randrange(steps - 1))            # the step boundary the kind is about
    if kind[0] == "R" and kind != "R256":
        b.pkt(3, at - 60 - 3)
        b.to(at + int(kind[1:]), lit=2)
    elif kind == "R256":
        b.pkt(0 if B == 256 else 7, 256 if B == 256 else 300)
    elif kind[0] == "L" and kind != "LL":
        x = int(kind[1:])
        if at + x + b.min_run > B:
            at = STEP
        b.pkt(2, at - 8 - 2)
        if at + x + b.min_run > B:
            # B = 256, x = 127: a packet's literals are followed by its run of >= 2 bytes, so no packet's stretch ends at byte 255.  The nearest form: the
            # TERMINATOR's literals from 8 bytes in front of the boundary to the block's end (property Lt: they cross by 128); L127 itself is in the B = 384 containers
            tail = "literals"
        else:
            b.pkt(8 + x, b.min_run)
    elif kind == "LL":
        b.pkt(4, 12 + rng.randrange(8))
        b.pkt(129 + rng.randrange(B - 129 - 40), b.min_run)
    elif kind == "E":
        b.pkt(3, at - 3)
        b.pkt(2, 30)
    elif kind == "T":
        b.pkt(9, 91)
        b.to(B, lit=5)
    elif kind == "H":
        for _ in range(14):
            b.pkt(rng.randrange(4), b.min_run, wide=True)
    elif kind == "D":
        while B - b.o > 24:
            b.pkt(rng.randrange(3), b.min_run)
    else:
        assert kind == "I"
        b.pkt(0, B)
    stream, out, headers, term = b.finish(form if kind == "T" else None, tail)
    return Block(kind, stream, out, b.events, term, headers)


def properties(blk, B):
    """The named properties a block HAS, read from where its packets lie (not from its label)."""
    have = set()
    bounds = range(STEP, B, STEP)
    for lit0, run0, end, _ in blk.events:
        for k in bounds:
            if run0 < k < end and end - k in CROSS:
                have.add(f"R{end - k}")
            if lit0 < k < run0 and run0 - k in CROSS:
                have.add(f"L{run0 - k}")
            if end == k:
                have.add("E")
        if end - run0 >= 256:
            have.add("R256")
        if run0 - lit0 > STEP:
            have.add("LL")
    last = blk.events[-1]
    if any(last[2] < k < B for k in bounds) and B - last[2] > STEP and len(blk.term.lit) == B - last[2]:
        have.add("Lt")
    if last[2] == B and B % STEP == 0 and not blk.term.lit:
        have.add("T")
    wide = [i for i, e in enumerate(blk.events) if e[3]]
    if len(wide) >= 12 and wide == list(range(wide[0], wide[0] + len(wide))):
        h = blk.headers[wide[0] : wide[-1] + 1]
        if h[-1][0] + h[-1][1] - h[0][0] > 140:
            have.add("H")
    if len(blk.events) >= B // 10:            # (the smallest run is 2 .. 6 bytes, 0 - 2 literals in front of it)
        have.add("D")
    if len(blk.events) == 1 and blk.events[0][2] == B:
        have.add("I")
    return have


_CACHE = {}


def container(codec, mixture, B, blocks):
    """(decoder_fixtures.Fixture, [Block]) -- fix.data is the writers' intended output.  Deterministic per arguments."""
    key = (codec.key, mixture, B, blocks)
    if key not in _CACHE:
        rng = random.Random(6151 * CODECS.index(codec) + 17 * B + blocks + (3 if mixture == "dense" else 0))
        kinds = list(MIXTURES[mixture])
        assert len(kinds) == F.WAVE
        rng.shuffle(kinds)
        kinds = (kinds + [("LL", "R16", "L17", "E", "D", "T")[CODECS.index(codec) % 6]])[:blocks]      # (65 blocks: the one active lane of the second wave)
        forms, t = last_forms(G.grammar(codec)), 2 * SHAPES.index((B, blocks))
        blks = []
        for kind in kinds:
            blks.append(build_block(codec, kind, B, rng, forms[t % len(forms)]))
            t += kind == "T"
        data = np.frombuffer(b"".join(x.out for x in blks), dtype=np.uint8)
        _CACHE[key] = (F.assemble(codec, mixture, B, data, kinds, [x.stream for x in blks]), blks)
    return _CACHE[key]


def _resize(stream, n=None, U=None):
    """The stream cut to n bytes, with a header that says so (and says U output bytes)."""
    s = bytearray(stream if n is None else stream[:n])
    struct.pack_into("<I", s, 4, len(s))
    if U is not None:
        struct.pack_into("<I", s, 0, U)
    return bytes(s)


def malformed_stream(codec, what, B, rng):
    """(stream, the output bytes a decoder can have produced in front of the fault)"""
    b = _Builder(codec, B, rng)
    g = b.g
    b.pkt(3, 60)
    if what == "cut_literal":
        b.pkt(100, b.min_run)
        stream = b.finish()[0]
        off, n = b.w.headers[1]
        return _resize(stream, off + n + 40), b.w.out[: 63 + 40]
    if what in ("cut_header_1", "cut_header_mid"):
        b.pkt(2, b.min_run, wide=True)
        stream = b.finish()[0]
        off, n = b.w.headers[1]
        return _resize(stream, off + (1 if what == "cut_header_1" else n // 2)), b.w.out[:63]
    if what == "early_end":
        stream = b.w.finish(G.Term(True, b"", "u16", "u32"))[0]
        return _resize(stream, U=B), b.w.out[:63]
    if what == "range_below_2":
        assert g.kind in ("lut", "short")
        b.pkt(77, b.min_run, wide=True)
        stream = bytearray(b.finish()[0])
        off, n = b.w.headers[1]
        at = bytes(stream[off : off + n]).find(struct.pack("<I", 77 + g.bias))
        assert at >= 0 and bytes(stream[off : off + n]).count(struct.pack("<I", 77 + g.bias)) == 1
        struct.pack_into("<I", stream, off + at, 1)
        return bytes(stream), b.w.out[:63]
    if what == "literal_leaves":
        b.pkt(77, b.min_run, wide=True)
        stream = bytearray(b.finish()[0])
        off, n = b.w.headers[1]
        field = 77 + g.bias
        field = struct.pack("<I", (field << 1) | 1 if g.range7 else field)
        big = 0x7FFFFF00 + g.bias
        at = bytes(stream[off : off + n]).rfind(field)
        assert at >= 0
        struct.pack_into("<I", stream, off + at, (big << 1) | 1 if g.range7 else big)
        return bytes(stream), b.w.out[:63]
    assert what == "no_terminator"
    b.to(B, lit=5)
    stream = b.finish()[0]
    return _resize(stream, b.w.headers[-1][0]), b.w.out[:B]


def malformed_container(codec, mixture, B, blocks, what):
    """The container of the same arguments with block VICTIM replaced by the malformed stream; fix.data holds the intended bytes of every OTHER block."""
    fix, _ = container(codec, mixture, B, blocks)
    rng = random.Random(7 * CODECS.index(codec) + B + blocks + MALFORMED.index(what))
    stream, _ = malformed_stream(codec, what, B, rng)
    streams = list(fix.streams)
    streams[VICTIM] = stream
    return F.assemble(codec, mixture, B, fix.data, fix.kinds, streams)


def window_ranges(fix):
    """Everything but the first and the last byte; from the last byte of a step of block 7 over the whole next block; the last byte."""
    B, U = fix.B, fix.U
    return [(1, U - 2), (7 * B + STEP - 1, B + 130), (U - 1, 1)]


def victim_window(fix):
    return VICTIM * fix.B - 10, fix.B + 20


def golden_key(codec, what, variant):
    """The recorded verdict is one per codec, malformed kind and decode variant: the parent said the same for every mixture, block size and block count (the
    recording run asserts it)."""
    return f"{codec.key}/{what}/{variant}"
