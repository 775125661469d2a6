"""The low-entropy streams written from their grammar (csrc/hsrle_rle8m.hip.h has the format), not by an encoder.

    unsectioned  [u32 compressedSize][u32 uncompressedSize][info][one stream]
    rle8m        [u32 compressedSize][u32 uncompressedSize][u32 sections][u32 end offset of section 0 .. sections - 2][info][section streams]
    info         32 flag bytes (bit s: symbol s is followed by a repeat code), u8 n (0 stands for 255), n symbols

A stream is a sequence of tokens: a symbol, and behind a flagged symbol the CODE of how many more of it follow.  The code of count c is the
symbol listed at position c; symbols that are not listed take the counts behind the list in ascending order (modulo 256); of two listings of
one symbol the last one counts (reference: rle8_low_entropy_cpu.c:569-600).  rle8m section k decodes to uncompressedSize / sections bytes, the
last one to the rest.

Three things live here: `tables` / `write_le` / `write_rle8m` (writers that check nothing), `model` (the sequential decoder in ten lines, for
well-formed streams) and `parse` (the same with every bound checked, the rule that failed by name, and a Counter of the forms a stream holds).
Behind them the fixtures of the decoder tests: tests/test_low_entropy_grammar.py decodes them on the CPU, tests/test_gpu_low_entropy_grammar.py
on the GPU, so both hold the same bytes."""
import functools
import random
import struct
from collections import Counter

import numpy as np

PIECE = 16384            # the unsectioned decoder cuts the stream every PIECE bytes (kLePiece, csrc/hsrle_capi_low_entropy.h)
WINDOW = 64              # stream bytes per decode step of a wave
CARRY_LIMIT = 1 << 16    # kLeCarryLimit: the backward scan in front of a piece gives up here

FORMS = ("cnt.0", "cnt.254", "code.flagged", "code.plain", "tok.same_again", "list.dup", "list.n0", "list.short", "list.unsorted", "code.unlisted",
         "flag.unused", "flags.1", "flags.256", "section.empty")


class Malformed(Exception):
    def __init__(self, rule):
        Exception.__init__(self, rule)
        self.rule = rule


# ------------------------------------------------------------------------------------------------------------------
# writers


def listed_count(listed, n_byte=None):
    """(the stored count byte, how many list entries a reader takes)"""
    n = (len(listed) & 0xFF) if n_byte is None else n_byte
    return n, (n or 255)


def tables(flags, listed, n_byte=None):
    """code -> count by the reference's rule: the last listing of a symbol wins, unlisted symbols take the following counts in ascending
    order modulo 256, a stored 0 means 255 listed symbols.  (`flags` plays no part: the argument keeps the writers' signature.)"""
    _, sc = listed_count(listed, n_byte)
    if len(listed) < sc:
        raise ValueError("the list is shorter than its count byte says")
    count_of = [None] * 256
    for k in range(sc):
        count_of[listed[k]] = k
    nxt = sc
    for sym in range(256):
        if count_of[sym] is None:
            count_of[sym] = nxt & 0xFF
            nxt += 1
    return count_of


def codes_of(count_of):
    """count -> the codes that stand for it, ascending (none: a position of the list that a later listing took over; two: the modulo)"""
    inv = [[] for _ in range(256)]
    for code, c in enumerate(count_of):
        inv[c].append(code)
    return inv


def info_bytes(flags, listed, n_byte=None):
    bits = bytearray(32)
    for s in flags:
        bits[s >> 3] |= 1 << (s & 7)
    n, _ = listed_count(listed, n_byte)
    return bytes(bits) + bytes([n]) + bytes(listed)


def body_bytes(flags, listed, tokens, n_byte=None):
    """tokens: (symbol, count, which code of that count) -- count None: the symbol alone; or the body's bytes as they are"""
    if isinstance(tokens, (bytes, bytearray)):
        return bytes(tokens)
    inv = codes_of(tables(flags, listed, n_byte))
    out = bytearray()
    for sym, count, which in tokens:
        out.append(sym)
        if count is not None:
            out.append(inv[count][which])
    return bytes(out)


def tokens_size(tokens):
    return sum(1 + (c or 0) for _, c, _ in tokens)


def write_le(flags, listed, tokens, n_byte=None, out_size=None, comp_size=None):
    """The unsectioned stream of `tokens` (or of a ready body).  out_size / comp_size: the header words, where they shall say something else."""
    body = body_bytes(flags, listed, tokens, n_byte)
    info = info_bytes(flags, listed, n_byte)
    if out_size is None:
        out_size = body_size(flags, tables(flags, listed, n_byte), body) if isinstance(tokens, (bytes, bytearray)) else tokens_size(tokens)
    size = 8 + len(info) + len(body)
    return struct.pack("<II", size if comp_size is None else comp_size, out_size) + info + body


def write_rle8m(flags, listed, sections, n_byte=None, out_size=None, comp_size=None, ends=None, section_count=None):
    """The rle8m stream of one token list (or ready body) per section, with its end-offset table.  ends: another table (sections - 1 words)."""
    bodies = [body_bytes(flags, listed, t, n_byte) for t in sections]
    info = info_bytes(flags, listed, n_byte)
    n = len(bodies)
    if out_size is None:
        count_of = tables(flags, listed, n_byte)
        out_size = sum(body_size(flags, count_of, b) for b in bodies)
    at = 12 + 4 * (n - 1) + len(info)
    table = []
    for b in bodies[:-1]:
        at += len(b)
        table.append(at)
    size = at + len(bodies[-1])
    table = table if ends is None else list(ends)
    return struct.pack(f"<III{len(table)}I", size if comp_size is None else comp_size, out_size, n if section_count is None else section_count, *table) + info + b"".join(bodies)


def body_size(flags, count_of, body):
    """output bytes of a well-formed body"""
    fl = [False] * 256
    for s in flags:
        fl[s] = True
    i, n, o = 0, len(body), 0
    while i < n:
        o += 1
        if fl[body[i]]:
            o += count_of[body[i + 1]]
            i += 2
        else:
            i += 1
    return o


# ------------------------------------------------------------------------------------------------------------------
# the sequential model (well-formed streams only) and the parser


def read_header(stream, sectioned):
    """(compressed size, uncompressed size, sections, section ends or None, flags as a list of 256 bools, code -> count, listed symbols, count byte, data start)"""
    size, out_size = struct.unpack_from("<II", stream, 0)
    sections = struct.unpack_from("<I", stream, 8)[0] if sectioned else 1
    info = 12 + 4 * (sections - 1) if sectioned else 8
    ends = list(struct.unpack_from(f"<{sections - 1}I", stream, 12)) if sectioned else []
    fl = [bool((stream[info + (s >> 3)] >> (s & 7)) & 1) for s in range(256)]
    n = stream[info + 32]
    listed = list(stream[info + 33 : info + 33 + (n or 255)])
    return size, out_size, sections, ends, fl, tables((), listed, n), listed, n, info + 33 + (n or 255)


def model(stream, sectioned):
    """What a well-formed stream decodes to: one token after the other, no questions asked."""
    size, _, _, ends, fl, count_of, _, _, at = read_header(stream, sectioned)
    out = bytearray()
    for end in ends + [size]:
        while at < end:
            b = stream[at]
            if fl[b]:
                out += bytes([b]) * (1 + count_of[stream[at + 1]])
                at += 2
            else:
                out.append(b)
                at += 1
    return bytes(out)


def parse(stream, sectioned):
    """(output, Counter of the forms the stream holds -- FORMS), or Malformed(rule)."""
    n_in = len(stream)
    if n_in < (12 if sectioned else 8):
        raise Malformed("header.short")
    size, out_size = struct.unpack_from("<II", stream, 0)
    if size > n_in:
        raise Malformed("size.above_buffer")
    sections = 1
    if sectioned:
        sections = struct.unpack_from("<I", stream, 8)[0]
        if sections == 0:
            raise Malformed("sections.zero")
    info = 12 + 4 * (sections - 1) if sectioned else 8
    if info + 33 > size:
        raise Malformed("info.past_stream")
    n = stream[info + 32]
    sc = n or 255
    if info + 33 + sc > size:
        raise Malformed("list.past_stream")
    data_start = info + 33 + sc
    fl = [bool((stream[info + (s >> 3)] >> (s & 7)) & 1) for s in range(256)]
    listed = list(stream[info + 33 : data_start])
    count_of = tables((), listed, n)
    is_listed = [False] * 256
    for s in listed:
        is_listed[s] = True

    forms = Counter()
    toks = Counter()                       # tokens per symbol
    out = bytearray()
    share = out_size // sections
    begin = data_start
    for k in range(sections):
        last = k + 1 == sections
        end = size if last else struct.unpack_from("<I", stream, 12 + 4 * k)[0]
        want = out_size - share * (sections - 1) if last else share
        if end > size:
            raise Malformed("section.end_above_size")
        if end < begin:
            raise Malformed("section.end_below_data" if k == 0 else "section.end_below_begin")
        if end == begin and sectioned:
            forms["section.empty"] += 1
        o_end = len(out) + want
        at, prev = begin, None
        while at < end:
            b = stream[at]
            at += 1
            if len(out) >= o_end:
                raise Malformed("out.over")
            toks[b] += 1
            if not fl[b]:
                out.append(b)
                prev = None
                continue
            if at >= end:
                raise Malformed("flagged.last_byte")
            code = stream[at]
            at += 1
            count = count_of[code]
            if len(out) + 1 + count > o_end:
                raise Malformed("count.past_share")
            out += bytes([b]) * (1 + count)
            forms["cnt.%d" % count] += 1
            forms["code.flagged" if fl[code] else "code.plain"] += 1
            if not is_listed[code]:
                forms["code.unlisted"] += 1
            if prev == b:
                forms["tok.same_again"] += 1
            prev = b
        if len(out) != o_end:
            raise Malformed("out.under")
        begin = end

    nflags = sum(fl)
    forms["flags.%d" % nflags] += 1
    if len(set(listed)) < len(listed):
        forms["list.dup"] += 1
    if n == 0:
        forms["list.n0"] += 1
    if any(not is_listed[s] for s in toks):                # an encoder lists every symbol that occurs
        forms["list.short"] += 1
    per = [toks[s] for s in listed]                        # ... in the order of their token counts, most first
    if any(a < b for a, b in zip(per, per[1:])):
        forms["list.unsorted"] += 1
    if any(fl[s] and toks[s] == 0 for s in range(256)):
        forms["flag.unused"] += 1
    return bytes(out), forms


# ------------------------------------------------------------------------------------------------------------------
# fixtures


class Header:
    """flags + list, and the code bytes of a count by whether their own value is flagged"""

    def __init__(self, flags, listed, n_byte=None):
        self.flags, self.listed, self.n_byte = frozenset(flags), list(listed), n_byte
        self.count_of = tables(flags, listed, n_byte)
        self.inv = codes_of(self.count_of)
        self.plain = [s for s in range(256) if s not in self.flags]

    def code(self, count, flagged=None):
        for c in self.inv[count]:
            if flagged is None or (c in self.flags) == flagged:
                return c
        raise KeyError((count, flagged))

    def le(self, body, **kw):
        return write_le(self.flags, self.listed, bytes(body), self.n_byte, **kw)

    def rle8m(self, bodies, **kw):
        return write_rle8m(self.flags, self.listed, [bytes(b) for b in bodies], self.n_byte, **kw)


def _listed_with(at, rest):
    """255 distinct symbols: position -> symbol as `at` says, the others from `rest` in order"""
    taken = set(at.values())
    pool = [s for s in rest if s not in taken]
    return [at[k] if k in at else pool.pop(0) for k in range(255)]


F0, F1, F2, F3, F4 = 0xF0, 0xF1, 0xF2, 0xF3, 0xF4
EDGE_FLAGS = (F0, F1, F2, F3, F4, 0x00, 0x80)
# HF: the codes of 0, 1, 254 are flagged values, those of 2, 3 are not.  HP: the other way round.
HF = Header(EDGE_FLAGS, _listed_with({0: F1, 1: F2, 254: F3, 2: 0x10, 3: 0x11}, range(1, 256)))
HP = Header(EDGE_FLAGS, _listed_with({0: 0x10, 1: 0x11, 254: 0x12, 2: F1, 3: F2}, range(1, 256)))


class Body(bytearray):
    """a stream body under construction; `h` names the codes"""

    def __init__(self, h):
        bytearray.__init__(self)
        self.h = h

    def plain(self, n):
        """n symbols without a flag (their values walk, so that a shifted output shows)"""
        p = self.h.plain
        self += bytes(p[(len(self) + j) % 61] for j in range(n))
        return self

    def pad_to(self, pos):
        assert len(self) <= pos, (len(self), pos)
        return self.plain(pos - len(self))

    def tok(self, sym, count, flagged=None):
        self.append(sym)
        self.append(self.h.code(count, flagged))
        return self

    def stretch(self, length):
        """`length` bytes in a row whose values are flagged: tokens of F0 with a flagged-valued code; an odd stretch ends with a symbol, whose
        code (its value not flagged) follows the stretch"""
        small = 0 if self.h is HF else 2
        for _ in range(length // 2):
            self.tok(F0, small, True)
        if length & 1:
            self.tok(F4, 3 if self.h is HF else 1, False)
        return self


def placements(h):
    """(name, front, emit) -- emit(body, E) writes from E - front on so that the named byte is stream byte E - 1"""
    flagged_codes = h is HF
    out = [("plain", 1, lambda b, E: b.plain(1))]
    for c in (0, 1, 254):
        out.append((f"sym.code{c}", 1, lambda b, E, c=c: b.tok(F2, c, flagged_codes)))
    out.append(("code", 2, lambda b, E: b.tok(F3, 3 if h is HF else 0, False)))
    out.append(("code.flagged_value", 2, lambda b, E: b.tok(F3, 0 if h is HF else 2, True)))
    for front in (1, 2, 127, 128, 129):
        for behind in (4, 5):
            out.append((f"stretch.{front}+{behind}", front, lambda b, E, L=front + behind: b.stretch(L)))
    return out


def edge_body(h, unit):
    """One body with every placement of `h` at an edge: multiples of `unit` stream bytes, far enough apart (unit 64: every fifth window edge)."""
    step = unit if unit >= 512 else unit * 5
    b = Body(h)
    E = step
    for name, front, emit in placements(h):
        b.pad_to(E - front)
        emit(b, E)
        b.plain(3)
        E += step
    return b.plain(70)


def sizes_body(h, n):
    """exactly n stream bytes: symbols, and tokens where they fit, the last one ending on the last byte"""
    b = Body(h)
    j = 0
    while len(b) < n:
        if n - len(b) >= 2 and j % 3 == 1:
            b.tok(F1 if j % 2 else F2, (j * 7) % 12, None)
        else:
            b.plain(1)
        j += 1
    assert len(b) == n
    return b


def lane0_code_only_body(h):
    """a window whose only repeat code is its lane 0 and that holds no flagged value: the symbol in lane 63 of the window before"""
    b = Body(h)
    b.pad_to(2 * WINDOW - 1)
    b.tok(F2, 3 if h is HF else 1, False)
    return b.plain(WINDOW - 1 + 40)


def whole_windows_body(h, length, lead):
    """a flagged-valued stretch of `length` bytes that starts `lead` bytes in front of a window edge"""
    b = Body(h)
    b.pad_to(3 * WINDOW - lead)
    b.stretch(length)
    return b.plain(9)


def limit_body(length, edge_piece=5):
    """a stretch of `length` flagged-valued bytes that ends right in front of a piece edge"""
    b = Body(HF)
    E = edge_piece * PIECE
    b.pad_to(E - length)
    b.stretch(length)
    return b.plain(100)


def one_stretch_body():
    """nothing but one stretch, long enough for a piece to start CARRY_LIMIT bytes into it"""
    return Body(HF).stretch(CARRY_LIMIT + PIECE)


def ladder_body(h=None):
    """packet lengths 1 .. 255, each at every output offset modulo 16"""
    h = h or LADDER
    b = Body(h)
    for length in range(1, 256):
        for _ in range(16):
            b.tok(F0, length - 1, None)
            b.plain((1 - length) % 16)           # packet + symbols = 1 modulo 16: the next packet starts one byte further
    return b


# every count has one code here: the identity list
LADDER = Header((F0,), list(range(255)))


def _random_tokens(h, rng, n, counts):
    toks, flags = [], sorted(h.flags)
    usable = [c for c in counts if h.inv[c]]
    for _ in range(n):
        if flags and (rng.random() < 0.6 or len(flags) == 256):
            c = rng.choice(usable)
            toks.append((rng.choice(flags), c, rng.randrange(len(h.inv[c]))))
        else:
            toks.append((rng.choice(h.plain), None, 0))
    return toks


@functools.lru_cache(maxsize=None)
def header_forms():
    """name -> (Header, tokens): one header per form of FORMS that concerns the header"""
    rng = random.Random(2304)
    small = [0, 0, 1, 2, 3, 7, 31, 32, 33, 254]
    perm = list(range(256))
    rng.shuffle(perm)
    out = {}

    def add(name, h, counts=small, n=300, first=()):
        out[name] = (h, list(first) + _random_tokens(h, rng, n, counts))

    add("plain_list", Header((1, 2, 3), perm[:255]))
    add("list.short", Header((5, 9), [9, 5, 200]), counts=list(range(0, 40)) + [254])
    add("list.unsorted", Header((5, 9), perm[:40]))
    # a symbol listed twice: the later listing wins, the earlier position has no code.  Both listings in one group of 64 positions (the table
    # builder takes 64 positions per step, one per lane), in neighbouring groups, and in the first and the last group; the duplicated symbols
    # are the codes that the tokens use
    others = iter([s for s in perm if not 0x21 <= s <= 0x25])
    dup = [None] * 255
    dup[3], dup[40] = 0x21, 0x21          # same step, later lane wins
    dup[50], dup[7] = 0x22, 0x22
    dup[63], dup[64] = 0x23, 0x23         # neighbouring steps
    dup[1], dup[254] = 0x24, 0x24         # first and last step
    dup[130], dup[131], dup[132] = 0x25, 0x25, 0x25
    dup = [next(others) if s is None else s for s in dup]
    hd = Header((0x21, 0x24, 7), dup)
    add("list.dup", hd, counts=[40, 50, 64, 254, 132, 0, 2], first=[(7, c, 0) for c in (40, 50, 64, 254, 132)])
    add("list.dup_short", Header((1, 2), [1, 2, 1, 2, 1, 1, 2]), counts=list(range(0, 30)))
    add("list.n0", Header((4, 250), perm[:255], n_byte=0))
    add("code.unlisted", Header((5,), [5, 6, 7, 8]), counts=[4, 5, 6, 100, 254])
    add("flag.unused", Header((5, 6, 222), perm[:255]))
    out["flag.unused"] = (out["flag.unused"][0], [t for t in out["flag.unused"][1] if t[0] != 222])     # 222 is flagged and never occurs
    add("flags.1", Header((0,), perm[:255]))
    add("flags.256", Header(range(256), perm[:255]), n=200)
    add("flags.256_n0", Header(range(256), list(range(255)), n_byte=0), n=200)
    add("flags.0", Header((), perm[:3]), n=150)
    return out


ALL_256_INPUT = b"".join(bytes([s]) * 3 for s in range(256)) * 3          # every encoder flags all 256 symbols on it


@functools.lru_cache(maxsize=None)
def le_fixtures():
    """name -> unsectioned stream (well formed)"""
    fx = {}
    for n in (1, 63, 64, 65, PIECE - 1, PIECE, PIECE + 1, 3 * PIECE + 7):
        fx[f"size.{n}"] = HF.le(sizes_body(HF, n))
    for tag, h in (("hf", HF), ("hp", HP)):
        fx[f"piece_edges.{tag}"] = h.le(edge_body(h, PIECE))
        fx[f"window_edges.{tag}"] = h.le(edge_body(h, WINDOW))
        fx[f"lane0_code_only.{tag}"] = h.le(lane0_code_only_body(h))
        for length, lead in ((130, 1), (131, 1), (131, 2)):
            fx[f"whole_windows.{tag}.{length}.{lead}"] = h.le(whole_windows_body(h, length, lead))
    fx["ladder"] = LADDER.le(ladder_body())
    for name, (h, toks) in header_forms().items():
        fx[f"form.{name}"] = write_le(h.flags, h.listed, toks, h.n_byte)
    return fx


@functools.lru_cache(maxsize=None)
def le_limit_fixtures():
    """name -> (unsectioned stream, decode attempts: 2 where a piece has CARRY_LIMIT flagged-valued bytes or more in front of it)"""
    fx = {}
    for length in (CARRY_LIMIT - 1, CARRY_LIMIT, CARRY_LIMIT + 1):
        fx[f"limit.{length}"] = (HF.le(limit_body(length)), 1 if length < CARRY_LIMIT else 2)
    fx["limit.one_stretch"] = (HF.le(one_stretch_body()), 2)
    return fx


@functools.lru_cache(maxsize=None)
def rle8m_fixtures():
    """name -> rle8m stream (well formed) for the wave kernel: the edge placements from each section's start, 1 / 2 / 3 / 64 sections, sections
    that end mid-window, on a window multiple, or hold nothing"""
    fx = {}
    for tag, h in (("hf", HF), ("hp", HP)):
        mid = bytes(edge_body(h, WINDOW))                                  # ends mid-window
        assert len(mid) % WINDOW != 0
        whole = mid + bytes(Body(h).plain((-len(mid)) % WINDOW))           # ends on a window multiple
        assert len(whole) % WINDOW == 0
        lane0 = bytes(lane0_code_only_body(h))
        for nsec in (1, 2, 3, 64):
            fx[f"edges.{tag}.{nsec}.mid"] = h.rle8m([mid] * nsec)
            # equal shares: every section holds the same tokens
            fx[f"edges.{tag}.{nsec}.multiple"] = h.rle8m([whole] * nsec)
        # sections of different bodies and equal output: the last section may be longer
        tail = bytes(Body(h).plain(body_size(h.flags, h.count_of, mid) + 3))
        fx[f"mixed.{tag}"] = h.rle8m([mid, bytes(Body(h).plain(body_size(h.flags, h.count_of, mid))), mid, tail])
        s = body_size(h.flags, h.count_of, lane0)
        fx[f"lane0_code_only.{tag}"] = h.rle8m([lane0, bytes(Body(h).plain(s)), lane0])
        for length, lead in ((130, 1), (131, 1), (131, 2)):
            w = bytes(whole_windows_body(h, length, lead))
            fx[f"whole_windows.{tag}.{length}.{lead}"] = h.rle8m([w, w])
    # uncompressedSize < sections: every section but the last is empty
    for nsec in (2, 3, 64):
        fx[f"empty_sections.{nsec}"] = HF.rle8m([b""] * (nsec - 1) + [bytes(Body(HF).tok(F2, 0, None))], out_size=1)
        fx[f"empty_sections.{nsec}.most"] = HF.rle8m([b""] * (nsec - 1) + [bytes(Body(HF).plain(nsec - 1))], out_size=nsec - 1)
    fx["ladder.2"] = LADDER.rle8m([bytes(ladder_body())] * 2)
    for name, (h, toks) in header_forms().items():
        for nsec in (1, 3):
            fx[f"form.{name}.{nsec}"] = write_rle8m(h.flags, h.listed, [toks] * nsec, h.n_byte)
    return fx


# ---- the lane kernel: 131 072 sections of 300 output bytes, 64 patterns tiled

LANE_SECTIONS, LANE_SHARE, LANE_PATTERNS = 131072, 300, 64
LANE_COUNTS = (0, 1, 15, 16, 17, 31, 32, 33, 254)


@functools.lru_cache(maxsize=None)
def lane_patterns():
    """64 section bodies of LANE_SHARE output bytes under LADDER's header (flagged: F0; the code of count c is c): runs that enter the 16-byte
    accumulator at every phase with each of LANE_COUNTS, a section of more than 32 tokens, a section without a flagged byte"""
    h = LADDER
    jobs = [(phase, c) for c in LANE_COUNTS for phase in range(16)]        # 144 (phase, count) pairs
    pats = []
    j = 0
    while len(pats) < LANE_PATTERNS - 2:
        b, o = Body(h), 0

        def sym(n):
            nonlocal o
            b.plain(n)
            o += n

        def run(c):
            nonlocal o
            b.tok(F0, c, None)
            o += 1 + c

        # as many of the jobs as fit: symbols up to the phase (the run's repeats start one byte behind its symbol), then the token
        while True:
            phase, c = jobs[j % len(jobs)]
            lead = (phase - (o + 1)) % 16
            if o + lead + 1 + c > LANE_SHARE:
                break
            sym(lead)
            run(c)
            j += 1
        sym(LANE_SHARE - o)
        pats.append(bytes(b))
    assert j >= len(jobs), "every (phase, count) pair is in a pattern"
    many = Body(h)                                                         # 100 tokens of 3 bytes: the ring is topped up more than once
    for _ in range(100):
        many.tok(F0, 2, None)
    pats.append(bytes(many))
    pats.append(bytes(Body(h).plain(LANE_SHARE)))                          # no flagged byte at all
    for p in pats:
        assert body_size(h.flags, h.count_of, p) == LANE_SHARE
    return pats


def lane_small():
    """the 64 patterns as one rle8m stream of 64 sections (what the parser reads)"""
    return LADDER.rle8m(lane_patterns())


@functools.lru_cache(maxsize=None)
def lane_stream():
    """(rle8m stream of LANE_SECTIONS sections: the 64 patterns tiled, its output) -- built with numpy"""
    pats = lane_patterns()
    reps = LANE_SECTIONS // LANE_PATTERNS
    body = np.frombuffer(b"".join(pats), dtype=np.uint8)
    lens = np.array([len(p) for p in pats], dtype=np.int64)
    info = info_bytes(LADDER.flags, LADDER.listed, LADDER.n_byte)
    data_start = 12 + 4 * (LANE_SECTIONS - 1) + len(info)
    ends = data_start + np.cumsum(np.tile(lens, reps))
    head = struct.pack("<III", int(ends[-1]), LANE_SECTIONS * LANE_SHARE, LANE_SECTIONS)
    stream = np.concatenate([np.frombuffer(head, dtype=np.uint8), ends[:-1].astype("<u4").view(np.uint8), np.frombuffer(info, dtype=np.uint8), np.tile(body, reps)])
    want = np.tile(np.frombuffer(model(lane_small(), True), dtype=np.uint8), reps)
    return stream.tobytes(), want.tobytes()


# ---- malformed streams: one per refusal rule of parse


def _patch32(stream, at, value):
    s = bytearray(stream)
    struct.pack_into("<I", s, at, value)
    return bytes(s)


@functools.lru_cache(maxsize=None)
def le_malformed():
    """name -> (unsectioned stream, the rule that refuses it).  The streams are long enough for the device entry point (41 bytes)."""
    h = HF
    good = Body(h).plain(40).tok(F2, 5, None).plain(30)
    n_out = body_size(h.flags, h.count_of, bytes(good))
    fx = {}
    s = h.le(good)
    fx["size.above_buffer"] = (_patch32(s, 0, len(s) + 1), "size.above_buffer")
    fx["info.past_stream"] = (struct.pack("<II", 40, 7) + bytes(60), "info.past_stream")
    fx["list.past_stream"] = (_patch32(s[: 8 + 33 + 100], 0, 8 + 33 + 100), "list.past_stream")
    fx["out.over"] = (h.le(good, out_size=n_out - 1), "out.over")
    fx["out.under"] = (h.le(good, out_size=n_out + 1), "out.under")
    fx["count.past_share"] = (h.le(Body(h).plain(40).tok(F2, 254, None), out_size=41 + 253), "count.past_share")
    fx["flagged.last_byte"] = (h.le(bytes(Body(h).plain(40)) + bytes([F2]), out_size=41), "flagged.last_byte")
    # ... in the last piece of several, whose last window is full: the stream ends on a pending code
    b = Body(h).pad_to(PIECE + 2 * WINDOW - 1)
    fx["pending_code.last_piece"] = (h.le(bytes(b) + bytes([F2]), out_size=len(b) + 1), "flagged.last_byte")
    # a piece that is not the last one decodes to one byte more / less than the header says: the total is what counts
    big = edge_body(h, PIECE)
    n_big = body_size(h.flags, h.count_of, bytes(big))
    fx["out.over.pieces"] = (h.le(big, out_size=n_big - 1), "out.over")
    fx["out.under.pieces"] = (h.le(big, out_size=n_big + 1), "out.under")
    return fx


@functools.lru_cache(maxsize=None)
def rle8m_malformed():
    """name -> (rle8m stream of 4 sections, the rule that refuses it)"""
    h = HF
    sec = bytes(Body(h).plain(40).tok(F2, 5, None).plain(30))
    n_sec = body_size(h.flags, h.count_of, sec)
    good = h.rle8m([sec] * 4)
    data_start = 12 + 4 * 3 + 33 + 255
    fx = {}
    fx["size.above_buffer"] = (_patch32(good, 0, len(good) + 1), "size.above_buffer")
    fx["sections.zero"] = (_patch32(good, 8, 0), "sections.zero")
    fx["info.past_stream"] = (struct.pack("<IIII", 40, 8, 2, 30) + bytes(60), "info.past_stream")
    fx["list.past_stream"] = (_patch32(good[: data_start - 100], 0, data_start - 100), "list.past_stream")
    e = [data_start + len(sec) * (k + 1) for k in range(3)]
    fx["section.end_below_data"] = (h.rle8m([sec] * 4, ends=[data_start - 1, e[1], e[2]]), "section.end_below_data")
    fx["section.end_below_begin"] = (h.rle8m([sec] * 4, ends=[e[0], e[0] - 1, e[2]]), "section.end_below_begin")
    fx["section.end_above_size"] = (h.rle8m([sec] * 4, ends=[e[0], len(good) + 1, e[2]]), "section.end_above_size")
    one_more = bytes(Body(h).plain(41).tok(F2, 5, None).plain(30))
    one_less = bytes(Body(h).plain(39).tok(F2, 5, None).plain(30))
    fx["out.over"] = (h.rle8m([sec, one_more, sec, sec], out_size=4 * n_sec), "out.over")
    fx["out.under"] = (h.rle8m([sec, one_less, sec, sec], out_size=4 * n_sec), "out.under")
    fx["out.over.last"] = (h.rle8m([sec, sec, sec, one_more], out_size=4 * n_sec), "out.over")
    past = bytes(Body(h).plain(40).tok(F2, 254, None))
    fx["count.past_share"] = (h.rle8m([sec, sec, past, sec], out_size=4 * n_sec), "count.past_share")
    last = bytes(Body(h).plain(n_sec - 1)) + bytes([F2])
    fx["flagged.last_byte"] = (h.rle8m([last, sec, sec, sec], out_size=4 * n_sec), "flagged.last_byte")
    full = bytes(Body(h).plain(2 * WINDOW - 1)) + bytes([F2])              # ... in lane 63 of a full window
    fx["flagged.last_byte.lane63"] = (h.rle8m([full, full], out_size=4 * WINDOW), "flagged.last_byte")
    return fx
