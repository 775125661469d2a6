"""Containers for the lazy run fill of the 8 bit packet loop of k_decode_blocks (hsrle_codecs.h: dec8_lazy_fill; a helper module like decode_loop_order_fixtures.py,
not a conftest).  The R section of a lazy kernel stores only the first 16-byte chunk of what it fills and marks the chunks that lie wholly inside the run; the flush
makes them.  So every stream here is PLACED with the writers of stream_grammar.py: where a run starts inside a chunk, how long it is and where it ends against the
16-byte chunks and the 128-byte steps is the point.  The containers come from hsrle_testlib.build_container.

Blocks of B = 384 / 4 096 bytes, 65 blocks (one full wave and one active lane of a second workgroup), the last block of 1, 127 or B - 1 bytes, every codec id of
one-byte symbols whose kernel has uncapped rounds (CODECS8: all but the two Short ids with a 3 / 7 symbol list).  Block kinds:
  S<off>L<len>   a run that starts at chunk offset off (0, 1, 15) and is len (15, 16, 17, 31, 32, 33, 111, 112, 113) bytes long, inside the block's second step
  E16  E128      a run that starts inside a chunk and ends exactly on a 16-byte / on a 128-byte boundary
  M3             one run over three whole steps and more (a whole step of the lane carries the mask 0xFE), from the middle of a chunk
  BB             two runs (of different symbols where packets carry one) back to back, no literal between, the second one over several chunks
  LRL            literal, run, literal inside ONE chunk
  C              a run from the middle of a chunk to the block's very end (cut there: the next block goes on with a run)
  F              the filler alone
  I              one run of the whole block: the neighbour that finishes every step in one packet
Two mixtures per wave (MIXTURES).  `sparse` fills the room around the placed run with runs (ratio <= 0.18: the 64-byte ring; nearly every chunk is lazy), `dense` with
literal stretches and short runs (ratio >= 0.40: the 128-byte ring).  The last block, of blen bytes, ends in a run that reaches its last byte (blen >= 127) -- the
chunk that run ends in is in no marked chunk and must still reach the output -- or is one literal byte.

Malformed streams (MALFORMED) replace ONE block (VICTIM):
  cut_after_marks   the stream is truncated right behind the header of a packet whose run has already marked chunks of the step when the lane finds that the next
                    header is missing: 2 literals, a run of 100 from the middle of the step's first chunk, then a header with nothing behind it
  run_then_garbage  behind a run over several chunks a literal count that leaves the stream (DEC_ERR_STREAM beside healthy lanes)
What the decoders must say about each is what the PARENT of the change said (tests/golden/decode_run_fill_status.json).
"""
import random
import struct

import numpy as np

import decode_loop_order_fixtures as L
import decoder_fixtures as F
import stream_grammar as G
from hsrle_testlib import CODECS, SHORT3, SHORT7

STEP, CHUNK = 128, 16
CODECS8 = [c for c in CODECS if c.S == 1 and c.family not in (SHORT3, SHORT7)]     # (those two have capped rounds: no full-row flush, no lazy fill)
BLOCK_SIZES = (384, 4096)
BLOCKS = 65
LAST_LENGTHS = lambda B: (1, 127, B - 1)
OFFSETS = (0, 1, 15)
LENGTHS = (15, 16, 17, 31, 32, 33, 111, 112, 113)
PLACED = tuple(f"S{o}L{n}" for o in OFFSETS for n in LENGTHS)
SPECIAL = PLACED + ("E16", "E128", "M3", "BB", "LRL", "C")
MIXTURES = {"sparse": SPECIAL + ("I",) * (64 - len(SPECIAL)),
            "dense": SPECIAL + ("F",) * 19 + ("I",) * (64 - len(SPECIAL) - 19)}
MALFORMED = ("cut_after_marks", "run_then_garbage")
VICTIM = 5
SUB_BLOCK = 128            # the entry-record decode: one lane per 128 output bytes, so lanes start in the middle of the long runs


class _Builder(L._Builder):
    def __init__(self, codec, B, rng, dense):
        super().__init__(codec, B, rng)
        self.dense = dense

    def run(self, lit, run, other=False):
        """a packet with `lit` literals and a run of exactly `run` bytes; other: of another symbol than the last packet's (where packets carry a symbol)"""
        if other and not self.g.stream_symbol:
            cur = self.w.state[0] if self.w.state else None
            self.syms = [s for s in self.syms if s != cur] or self.syms
        self.pkt(lit, run)
        self.syms = F._symbols(random.Random(len(self.w.s)), 1) if other else self.syms

    def fill_to(self, pos):
        """output bytes up to position pos: one run behind two literals (sparse), or literal stretches with short runs between (dense)"""
        while pos - self.o > 0:
            left = pos - self.o
            if left < self.min_run + 2:                       # too little for a packet's run: the next packet's literals take it
                return left
            if not self.dense or left < 40:
                self.pkt(2 if left >= self.min_run + 2 else 0, left - 2)
            else:
                lit = min(self.rng.randrange(30, 90), left - self.min_run)
                run = min(self.min_run + self.rng.randrange(6), left - lit)
                if left - lit - run < self.min_run + 2:
                    lit = left - run
                self.pkt(lit, run)
        return 0


def build_block(codec, kind, B, rng, dense, blen=None):
    """A Block (decode_loop_order_fixtures.Block) of blen (default B) output bytes."""
    blen = B if blen is None else blen
    b = _Builder(codec, blen, rng, dense)
    at = STEP                                                 # the placed run lies in the second step (B = 4 096: somewhere behind it)
    if B > 3 * STEP:
        at = STEP * rng.randrange(1, B // STEP - 2)
    if blen < B:
        # the last block of a buffer: a run that reaches its last byte from the middle of a chunk, or one literal byte
        if blen >= 100:
            lit = b.fill_to(blen - 100 - 3)
            b.run(lit + 3, 100)
    elif kind in PLACED:
        off, n = int(kind[1 : kind.index("L")]), int(kind[kind.index("L") + 1 :])
        start = at + CHUNK + off
        lit = b.fill_to(start - 1)
        b.run(lit + 1, n, other=True)
    elif kind in ("E16", "E128"):
        end = at + STEP if kind == "E128" else at + 5 * CHUNK
        start = at + CHUNK + 7
        lit = b.fill_to(start - 2)
        b.run(lit + 2, end - start, other=True)
    elif kind == "M3":
        lit = b.fill_to(at - STEP + 9 - 3)
        b.run(lit + 3, 3 * STEP + 40 if B > 3 * STEP else B - (at - STEP + 9), other=True)
    elif kind == "BB":
        lit = b.fill_to(at + 5 - 2)
        b.run(lit + 2, 21, other=True)
        b.run(0, 70, other=True)
    elif kind == "LRL":
        lit = b.fill_to(at + CHUNK)
        b.run(lit + 3, b.min_run, other=True)
        b.run(4, 40, other=True)
    elif kind == "C":
        lit = b.fill_to(B - 90 - 3)
        b.run(lit + 3, 90, other=True)
    elif kind == "I":
        b.pkt(0, B)
    else:
        assert kind == "F"
    if blen == B and kind not in ("I", "C", "M3") or (kind == "M3" and B > 3 * STEP):
        lit = b.fill_to(B)
        assert lit == 0 or b.o + lit == B
        left = lit
    else:
        left = blen - b.o
    term = G.Term(left == 0, rng.randbytes(left), "u32", "u32")
    stream, out, headers = b.w.finish(term)
    assert len(out) == blen, (kind, len(out), blen)
    return L.Block(kind, stream, out, b.events, term, headers)


def properties(blk, blen):
    """The named forms a block HAS, read from where its packets lie (not from its label): the test counts them over a container."""
    have = set()
    ev = blk.events
    for i, (lit0, run0, end, _) in enumerate(ev):
        n, off = end - run0, run0 % CHUNK
        if off in OFFSETS and n in LENGTHS:
            have.add(f"S{off}L{n}")
        if off and n >= CHUNK and end % CHUNK == 0:
            have.add("E16")
        if off and n >= CHUNK and end % STEP == 0 and end < blen:
            have.add("E128")
        if any(run0 <= k and k + STEP <= end for k in range(STEP, blen, STEP)) and off and n >= 3 * STEP - off:
            have.add("M3")
        if i and run0 == lit0 and ev[i - 1][2] == lit0 and ev[i - 1][2] > ev[i - 1][1] and n >= 2 * CHUNK:
            have.add("BB")
        if i and lit0 // CHUNK == run0 // CHUNK == (end + 1) // CHUNK and run0 > lit0 and i + 1 < len(ev) and ev[i + 1][1] > end:
            have.add("LRL")
        if end == blen and off and n >= 2 * CHUNK:
            have.add("C" if blen % CHUNK == 0 else "Ct")             # Ct: ... and the block's end lies inside a chunk (the tail bytes come from that run)
    if len(ev) == 1 and ev[0][1] == 0 and ev[0][2] == blen:
        have.add("I")
    return have


def lazy_chunks(blk):
    """How many 16-byte chunks of the block's output lie wholly inside a run and behind the chunk that run's step segment starts in: what a lazy kernel marks."""
    n = 0
    for _, run0, end, _ in blk.events:
        p = run0
        while p < end:
            seg_end = min(end, (p // STEP + 1) * STEP)
            n += max(seg_end // CHUNK - p // CHUNK - 1, 0)
            p = seg_end
    return n


_CACHE = {}


def container(codec, mixture, B, last_len):
    """(decoder_fixtures.Fixture, [Block]) of BLOCKS blocks, the last one of last_len bytes -- fix.data is the writers' intended output.  Deterministic."""
    key = (codec.key, mixture, B, last_len)
    if key not in _CACHE:
        rng = random.Random(8191 * CODECS.index(codec) + 31 * B + last_len + (7 if mixture == "dense" else 0))
        kinds = list(MIXTURES[mixture])
        assert len(kinds) == F.WAVE
        rng.shuffle(kinds)
        # (a C block's run is cut by the block's end: the block behind it begins with a run -- I, or any block of the sparse mixture)
        kinds = (kinds + ["T"])[:BLOCKS]
        dense = mixture == "dense"
        blks = [build_block(codec, k, B, rng, dense, last_len if i == BLOCKS - 1 else None) for i, k in enumerate(kinds)]
        data = np.frombuffer(b"".join(x.out for x in blks), dtype=np.uint8)
        _CACHE[key] = (F.assemble(codec, mixture, B, data, kinds, [x.stream for x in blks]), blks)
        while len(_CACHE) > 8:
            _CACHE.pop(next(iter(_CACHE)))
    return _CACHE[key]


def _resize(stream, n=None, U=None):
    s = bytearray(stream if n is None else stream[:n])
    struct.pack_into("<I", s, 4, len(s))
    if U is not None:
        struct.pack_into("<I", s, 0, U)
    return bytes(s)


def malformed_stream(codec, what, B, rng):
    b = _Builder(codec, B, rng, False)
    g = b.g
    b.run(2, STEP - 2 + 9)                                   # the second step begins in the middle of this run ...
    b.run(2, 100, other=True)                                # ... 2 literals, then a run from byte 11 of the step's first chunk over 6 chunks
    if what == "cut_after_marks":
        b.run(3, 20, other=True)
        off, n = b.w.headers[2]
        b.fill_to(B)
        stream = b.w.finish(G.Term(True, b"", "u32", "u32"))[0]
        return _resize(stream, off + n)                      # the third packet's header is the stream's end: its 3 literals are missing
    assert what == "run_then_garbage"
    b.pkt(77, b.min_run, wide=True)
    off, n = b.w.headers[2]
    b.fill_to(B)
    stream = bytearray(b.w.finish(G.Term(True, b"", "u32", "u32"))[0])
    field = 77 + g.bias
    field = struct.pack("<I", (field << 1) | 1 if g.range7 else field)
    big = 0x7FFFFF00 + g.bias
    at = bytes(stream[off : off + n]).rfind(field)
    assert at >= 0
    struct.pack_into("<I", stream, off + at, (big << 1) | 1 if g.range7 else big)
    return bytes(stream)


def malformed_container(codec, mixture, B, what):
    """The container (last block B - 1 bytes) with block VICTIM replaced by the malformed stream; fix.data holds the intended bytes of every OTHER block."""
    fix, _ = container(codec, mixture, B, B - 1)
    rng = random.Random(11 * CODECS.index(codec) + B + MALFORMED.index(what))
    streams = list(fix.streams)
    streams[VICTIM] = malformed_stream(codec, what, B, rng)
    return F.assemble(codec, mixture, B, fix.data, fix.kinds, streams)


def window_ranges(fix):
    """Everything but the first and the last byte; from the last byte of a step of block 7 over the whole next block; the last byte."""
    B, U = fix.B, fix.U
    return [(1, U - 2), (7 * B + STEP - 1, B + 130), (U - 1, 1)]


def victim_window(fix):
    return VICTIM * fix.B - 10, fix.B + 20


def golden_key(codec, what, variant):
    return f"{codec.key}/{what}/{variant}"
