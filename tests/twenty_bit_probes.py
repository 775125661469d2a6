"""Inputs that put the reference's 20-bit range rule in reach (plain Python and numpy; no GPU, no reference needed).

The LUT, Short and Greedy encoders (and rle8_single_short) store a run only if it pays for its header, and the reference steps that penalty
at 20 bits: a range or a stored count above 0xFFFFF costs 4, not 2 (reference: src/rleX_Xsl.h:130, src/rleX_Xsl_short.h:197).  The step is
only reachable with more than 1 MiB of literals in front of a run, or with a run of more than 2^20 symbols.

A range PROBE is
    separator   SEP symbols of one symbol: a run every encoder state stores and every many-lane path cuts behind (300 symbols in a
                monolithic input; 20 in a container block, where 300 symbols of 3 .. 8 bytes would not leave room for the gap) -- the
                probe's own symbol for the `listed` variant (the run then finds its symbol at the front of the list), 0x33 .. for `new`
    gap         filler bytes: range = gap + 2
    run         `count` BYTES of the probe's symbol (S bytes: A1 A2 .., B1 B2 .., ..)
    tail        120 filler bytes
and the COUNT probe a run whose stored count exceeds 0xFFFFF behind a 40-byte gap.  The filler has no equal bytes at distances 1 .. 16 and no
two neighbours that differ by one, so it holds no run of any width and no two bytes of a probe symbol.

Which counts flip between range T = 0xFFFFF and T + 1 is not typed in here: tests/golden/make_twenty_bit_golden.py finds them with the
compiled reference and records them in tests/golden/twenty_bit_probes.json, which plan() reads.
"""
import functools
import hashlib
import json
import os

import numpy as np

from hsrle_testlib import CODECS, GREEDY1, GREEDY3, GREEDY7, LUT3, LUT7, SHORT0, SHORT1, SHORT3, SHORT7, SINGLE_SHORT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "twenty_bit_probes.json")

T = 0xFFFFF
GAPS = (T - 2, T - 1)                      # range T and range T + 1
SEP_MONO, SEP_BLOCK = 300, 20              # separator symbols
TAIL = 120
COUNT_GAP = 40
MONO_MAX = 12 << 20
BLOCK = (1 << 20) + 1024
VARIANTS = ("listed", "new")

_RULE_FAMILIES = (LUT3, LUT7, SHORT0, SHORT1, SHORT3, SHORT7, GREEDY1, GREEDY3, GREEDY7, SINGLE_SHORT)
RULE_CODECS = [c for c in CODECS if c.family in _RULE_FAMILIES]     # the 82 codecs whose encoders have the rule
assert len(RULE_CODECS) == 82


def is_lut(codec):
    return codec.family in (LUT3, LUT7)


def is_chunk_mode_short(codec):
    """Short with no list or a one-symbol list (hsrle_codecs.h: chunk_mode): the codecs whose monolithic chunks go to the windowed encoder."""
    return codec.family in (SHORT0, SHORT1)


def stored_count(codec, count):
    """The reference's storedCount of a run of `count` bytes (rleX_Xsl.h:124-128, rleX_Xsl_short.h:171-175)."""
    S = codec.S
    mins = 3 if is_lut(codec) else (S + 2 if codec.family == SHORT0 else 2)
    return count // S - mins // S + 2 if codec.aligned else count - mins + 2


def count_probe_bytes(codec):
    """Length of the count probe's run: (0xFFFFF + 3) symbols for the sym-aligned codecs; for the others that many bytes plus S, because a
    Short codec without a list subtracts S from a byte count (stored_count) and (0xFFFFF + 3) bytes alone would stay at or below 0xFFFFF."""
    n = (T + 3) * codec.S if codec.aligned else T + 3 + codec.S
    assert stored_count(codec, n) > T
    return n


def count_candidates(S):
    return range(2, 6 * S + 25 + 1)


def filler(n, start=0):
    i = np.arange(start, start + n, dtype=np.int64)
    return ((37 * i + 101 * (i // 256)) & 0xFF).astype(np.uint8)


def symbol(S, j):
    """Probe symbol number j: A1 A2 .. for 0, B1 B2 .. for 1, ..."""
    return np.array([(0xA1 + 0x10 * j + k) & 0xFF for k in range(S)], dtype=np.uint8)


@functools.lru_cache(maxsize=16)
def _filler_between(n, before, after):
    """n filler bytes whose first byte is not `before` and whose last byte is none of `after` (a run must neither grow nor start early).
    (cached: callers only read it)"""
    for start in range(512):
        f = filler(n, start)
        if n == 0 or (int(f[0]) != before and int(f[-1]) not in after):
            return f
    raise AssertionError("no filler phase fits")


def _run(sym, count):
    return np.tile(sym, count // sym.size + 1)[:count]


def build_probe(S, variant, count, gap, sym_index=0, sep=SEP_MONO, size=None):
    """`size`: the tail is as long as it takes to fill so many bytes (at least TAIL)."""
    sym = symbol(S, sym_index)
    sep_sym = sym if variant == "listed" else np.full(S, 0x33, dtype=np.uint8)
    run = _run(sym, count)
    tail = TAIL if size is None else size - (sep * S + gap + count)
    assert tail >= TAIL
    # (the tail ends on no byte that the separator of a probe behind it could start with: a separator one byte early moves a sym-aligned range)
    parts = [np.tile(sep_sym, sep), _filler_between(gap, int(sep_sym[0]), (int(sym[-1]),)), run,
             _filler_between(tail, int(sym[count % S]), (0x33, int(symbol(S, 0)[-1])))]
    return np.concatenate(parts)


def build_count_probe(codec, sym_index=0):
    return build_probe(codec.S, "listed", count_probe_bytes(codec), COUNT_GAP, sym_index)


class Probe:
    def __init__(self, variant, count, gap, sym_index):
        self.variant, self.count, self.gap, self.sym_index = variant, count, gap, sym_index

    def key(self):
        return (self.variant, self.count, self.gap, self.sym_index)


def probe_list(S, flips):
    """The range probes of one codec from its flipping counts {variant: [counts]}, in the order in which the inputs take them: first the pair
    (c*, T - 2), (c*, T - 1) of each variant, then (c+ + 1, T - 1) and (c* - 1, T - 2); a variant without a flip has one pair at 2 S + 2.
    Every `listed` probe (and the count probe) has symbol 0; every `new` probe a symbol of its own, so that it is new in a concatenation too."""
    pairs, rest = [], []
    for variant in VARIANTS:
        f = sorted(flips.get(variant, []))
        if f:
            pairs += [(variant, f[0], T - 2), (variant, f[0], T - 1)]
            rest += [(variant, f[-1] + 1, T - 1), (variant, f[0] - 1, T - 2)]
        else:
            pairs += [(variant, 2 * S + 2, T - 2), (variant, 2 * S + 2, T - 1)]
    out, nxt = [], 1
    for variant, count, gap in pairs + rest:
        out.append(Probe(variant, count, gap, 0 if variant == "listed" else nxt))
        nxt += variant == "new"
    return out


def mono_input(codec, probes):
    """(input, indices of the range probes in it): the count probe, then as many range probes, in probe_list's order, as fit below MONO_MAX.
    Greedy codecs: the first pair only -- the many-lane monolithic encode finds no cut in these inputs for the Greedy encoders of 2, 4, 6 and 8
    byte symbols (hsrle_compress_mono_dev reports one chunk), so ONE lane encodes the whole input, at about 1.5 s per MiB of filler."""
    parts = [build_count_probe(codec)]
    size, used = parts[0].size, []
    for i, p in enumerate(probes[: 2 if codec.family in (GREEDY1, GREEDY3, GREEDY7) else None]):
        d = build_probe(codec.S, p.variant, p.count, p.gap, p.sym_index)
        if size + d.size > MONO_MAX:
            break
        parts.append(d)
        size += d.size
        used.append(i)
    return np.concatenate(parts), used


def container_input(codec, probes):
    """One range probe per block of BLOCK bytes, each block filled to its end with filler."""
    return np.concatenate([build_probe(codec.S, p.variant, p.count, p.gap, p.sym_index, sep=SEP_BLOCK, size=BLOCK) for p in probes])


def sha(stream):
    return hashlib.sha256(bytes(stream)).hexdigest()


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def plan(codec, golden=None):
    """The probes of `codec` as the golden file records them."""
    g = (golden or load_golden())["codecs"][codec.key]
    return [Probe(e["variant"], e["count"], e["gap"], e["symbol"]) for e in g["probes"]]
