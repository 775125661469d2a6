"""A model of what the low-entropy / rle8m ENCODERS count and decide, and inputs built around the places where they decide.

The encoders' statistics pass (oracle/hsrle_oracle.c, le_get_info_ex; csrc/hsrle_rle8m.hip.h: k_rle8m_stats_wave, k_le_scan_last, k_le_stats_fixup) gives
prob[256] and pcount[256]; the table pass (k_rle8m_info) uses them in three comparisons only: a flag (prob / pcount >= 2), an argmax for the
only_max_frequency forms (prob / pcount > 2, largest prob - 2 pcount, first wins) and an ordering by pcount (ties: lower symbol first).  A count that is off by
one changes the stream only where it crosses one of those, so the inputs here SIT on them:

  stats(data, max_len)            the counts, vectorised numpy (maximal runs from np.diff)
  tables(prob, pcount, only_max)  flags, symbol order, count byte -- with the quirk that 256 used symbols give a count byte of 0 and 255 listed symbols
  header_bytes(...)               the info bytes of a stream header from those tables
  fixtures_*()                    A1 tie probes for pcount, A2 threshold probes for prob, A3 scan / grid edges, A4 alphabets, A5 cut edges (k_le_cuts)

Every A1 / A2 probe carries `moves`: (only_max, "prob" | "pcount", symbol, +-1) -- moving that model count by one must change tables(...); a probe for
which it does not is a bug of the fixture (tests/test_low_entropy_stats.py asserts it).  Pieces: the statistics kernels work on 4 KiB pieces of the input,
the cut finder on 16 KiB pieces."""
import numpy as np

P4 = 4096            # the statistics kernels' piece
G16 = 16384          # the cut finder's piece (kLePiece)
SMALL = 5 * P4 + 77  # the size of a small probe where nothing asks for more
_FILL = np.arange(96, 157, dtype=np.uint8)   # 61 filler symbols: the period is no divisor of a piece


def as_array(data):
    return data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------
# the model


def stats(data, max_len):
    """(prob, pcount) as uint32[256]: a maximal run of length L adds L to prob and L // max_len + 1 to pcount; the run that reaches the end of the input adds 1
    to pcount, whatever its length (hsrle_oracle.c:1385-1405; the reference's pcount[0] = 0xFFFFFFFF start-up wraps back to 0 at the first byte)."""
    d = as_array(data)
    n = d.size
    assert n > 0
    starts = np.concatenate(([0], np.flatnonzero(np.diff(d)) + 1))
    lens = np.diff(np.concatenate((starts, [n])))
    syms = d[starts]
    tokens = lens // max_len + 1
    tokens[-1] = 1
    prob = np.bincount(syms, weights=lens, minlength=256).astype(np.uint64)          # (exact: far below 2^53)
    pcount = np.bincount(syms, weights=tokens, minlength=256).astype(np.uint64)
    return (prob & 0xFFFFFFFF).astype(np.uint32), (pcount & 0xFFFFFFFF).astype(np.uint32)


def tables(prob, pcount, only_max):
    """(flags uint8[256], order uint8[256], symbol_count byte) by the rule of hsrle_oracle.c:1407-1448.  order: the used symbols by falling pcount (ties: the
    lower symbol first), the unused ones behind in rising order; symbol_count: the used symbols as a uint8 (256 -> 0)."""
    prob = np.asarray(prob).astype(np.int64)
    pcount = np.asarray(pcount).astype(np.int64)
    used = pcount > 0
    ratio = prob // np.maximum(pcount, 1)
    flags = np.zeros(256, dtype=np.uint8)
    if not only_max:
        flags[used & (ratio >= 2)] = 1
    else:
        saved = np.where(used & (ratio > 2), (prob - 2 * pcount) & 0xFFFFFFFF, 0)   # (uint32 arithmetic, as in the reference)
        if saved.max() > 0:
            flags[int(np.argmax(saved))] = 1                                        # the first of the largest
    syms = np.arange(256)
    u = syms[used]
    u = u[np.lexsort((u, -pcount[u]))]
    order = np.concatenate((u, syms[~used])).astype(np.uint8)
    return flags, order, int(u.size) & 0xFF


def header_bytes(flags, order, symbol_count):
    """The info bytes of a stream: 32 bytes of flags, the count byte, the listed symbols (a count byte of 0 lists 255)."""
    return np.packbits(flags, bitorder="little").tobytes() + bytes([symbol_count]) + order[: symbol_count or 255].tobytes()


def model_header(data, max_len, only_max):
    return header_bytes(*tables(*stats(data, max_len), only_max))


def moved(prob, pcount, which, sym, delta):
    """The counts with one of them moved by delta."""
    prob, pcount = prob.astype(np.int64), pcount.astype(np.int64)
    (prob if which == "prob" else pcount)[sym] += delta
    return prob, pcount


# ------------------------------------------------------------------------------------------------------------------
# building inputs


class Fixture:
    def __init__(self, name, data, max_len=None, moves=()):
        self.name, self.data, self.max_len, self.moves = name, data, max_len, tuple(moves)

    def __repr__(self):
        return self.name

    @property
    def bytes(self):
        return self.data.tobytes()


def filler(n):
    """n bytes without a run (61 symbols in turn: none of them is ever flagged, prob == pcount)."""
    return np.resize(_FILL, n)


def compose(n, runs, lone=()):
    """n filler bytes with runs = (symbol, start, length) written into them and lone = (symbol, width, count): `count` isolated runs of `width` bytes of
    the symbol, put into the filler from the front on, a filler byte between any two of them and next to every run."""
    d = filler(n)
    free = np.ones(n, dtype=bool)
    for sym, start, length in runs:
        assert 0 <= start and length > 0 and start + length <= n, (sym, start, length, n)
        assert free[max(start - 1, 0) : min(start + length + 1, n)].all(), "runs touch"
        d[start : start + length] = sym
        free[start : start + length] = False
    edges = np.flatnonzero(np.diff(np.concatenate(([0], free.view(np.uint8), [0])).astype(np.int8)))
    gaps = [[int(a) + 1, int(b) - 1] for a, b in zip(edges[0::2], edges[1::2])]   # usable [from, to): the gap's first and last byte stay filler
    for sym, width, count in lone:
        for g in gaps:
            if count == 0:
                break
            k = min(count, max(0, (g[1] - g[0])) // (width + 1))
            if k == 0:
                continue
            at = g[0] + np.arange(k) * (width + 1)
            for j in range(width):
                d[at + j] = sym
            g[0] += k * (width + 1)
            count -= k
        assert count == 0, "no room for the isolated bytes"
    return d


def _size(span, lone, mod=77):
    """The smallest k * 4096 + mod, k >= 5, with room for `span` bytes of runs and the isolated bytes."""
    need = span + 4 + sum((w + 1) * c for _, w, c in lone)
    return max(5, -(-(need - mod) // P4)) * P4 + mod


def _tokens(length, m, final):
    return 1 if final else length // m + 1


def _place(x, start, length, lone, final_mod):
    """The input of a probe.  final_mod given: the run ends the input, whose size is final_mod modulo 4096 (`start` is not used)."""
    if final_mod is None:
        return compose(_size(start + length, lone), [(x, start, length)], lone)
    n = _size(length, lone, final_mod)
    return compose(n, [(x, n - length, length)], lone)


def tie_probe(name, m, x, y, start, length, final_mod=None, extra=0):
    """A1: a run of x at [start, start + length), and y as exactly pcount[x] + extra isolated bytes."""
    final = final_mod is not None
    cx = _tokens(length, m, final)
    lone = [(y, 1, cx + extra)]
    data = _place(x, start, length, lone, final_mod)
    if extra == 0:
        move = ("pcount", x, -1 if x < y else +1)    # a tie: the lower symbol stands first.  x < y: one less and y passes; x > y: one more and x passes
    else:
        assert extra == 1 and x < y
        move = ("pcount", x, +1)                     # y leads by one: one more is a tie, which x wins
    return Fixture(name, data, m, [(0, *move), (1, *move)])


def _pad_to(length, c, T, e):
    """Isolated (singles, pairs) of the run's symbol that make prob == T * pcount - e: a single adds 1 to both, a pair 2 to prob and 1 to pcount."""
    k = length - T * c + e
    assert k >= 0
    if T == 2:
        return k, 0
    assert T == 3
    return (k - k % 2) // 2, k % 2


def threshold_probe(name, m, x, start, length, T, e, final_mod=None):
    """A2: the run of A1 with x padded so that prob[x] == T * pcount[x] - e.  T = 2: the flag of the regular forms (e = 0 set, e = 1 clear); T = 3: whether x
    may carry the repeat codes of the only_max forms at all."""
    final = final_mod is not None
    singles, pairs = _pad_to(length, _tokens(length, m, final), T, e)
    lone = [(x, 1, singles), (x, 2, pairs)]
    data = _place(x, start, length, lone, final_mod)
    p, c = stats(data, m)
    assert int(p[x]) == T * int(c[x]) - e
    only_max = 1 if T == 3 else 0
    up = +1 if e else -1                             # towards the other side of the threshold
    return Fixture(name, data, m, [(only_max, "prob", x, up), (only_max, "pcount", x, -up)])


def saved_probe(name, m, x, z, start, length, lead):
    """A2, only_max: x (the probed run) and z (a run of the same length elsewhere) with saved[x] == saved[z] + lead, lead in {0, -1, +1}, set with one more
    isolated byte (saved - 1) of the one or the other.  The cases are the four in which one step of prob[x] changes the winner."""
    zstart = start + length + 10 + 3 * m
    lone = [(x, 1, 1 if lead < 0 else 0), (z, 1, 1 if lead > 0 else 0)]
    data = compose(_size(zstart + length, lone), [(x, start, length), (z, zstart, length)], lone)
    p, c = stats(data, m)
    sx, sz = int(p[x]) - 2 * int(c[x]), int(p[z]) - 2 * int(c[z])
    assert sx == sz + lead and int(p[x]) // int(c[x]) > 2 and int(p[z]) // int(c[z]) > 2
    step = {(True, 0): -1, (False, 0): +1, (True, -1): +1, (False, +1): -1}[(x < z, lead)]
    return Fixture(name, data, m, [(1, "prob", x, step)])


MAX_LENS = (255, 32)
LO, HI = 60, 61      # the probed symbol and its comparator, either way round


def _scenarios(m):
    for start in (P4 - m, P4 - 1, P4, P4 + 1, 2 * P4 - 2 * m):
        for length in (m - 1, m, m + 1, P4, P4 + m, 2 * P4 + 3):
            yield start, length


def _final_scenarios(m):
    """x as the input's final run: n a multiple of 4096, n % 4096 == 1, n % 4096 == 77; runs that begin in the last piece and in an earlier one."""
    for mod in (0, 1, 77):
        for length in (5, m - 1, m, m + 1, P4 + m, 2 * P4 + 3):
            yield mod, length


def fixtures_a1():
    """Tie probes for pcount: runs that begin or end on a piece edge, token boundaries on, before and behind an edge, runs over one, two and three pieces."""
    out = []
    for m in MAX_LENS:
        for start, length in _scenarios(m):
            for x, y in ((LO, HI), (HI, LO)):
                out.append(tie_probe(f"a1.m{m}.s{start}.l{length}.{'lo' if x < y else 'hi'}", m, x, y, start, length))
        for mod, length in _final_scenarios(m):
            for x, y in ((LO, HI), (HI, LO)):
                out.append(tie_probe(f"a1.final.m{m}.n%{mod}.l{length}.{'lo' if x < y else 'hi'}", m, x, y, None, length, final_mod=mod))
        for length in (m - 1, m, P4 + m):
            # the input's first byte: 0 (counted from the start), and another symbol with 0 only later (the reference's pcount[0] start-up wrap)
            out.append(tie_probe(f"a1.first0.m{m}.l{length}.less", m, 0, 1, 0, length))
            out.append(tie_probe(f"a1.first0.m{m}.l{length}.more", m, 0, 1, 0, length, extra=1))
            out.append(tie_probe(f"a1.first7.m{m}.l{length}.zero_later", m, 7, 0, 0, length))
    return out


def tie_probes_small():
    """The A1 probes of 5 * 4096 + 77 bytes (whose run does not end the input)."""
    return [f for f in fixtures_a1() if f.data.size == SMALL and not f.name.startswith("a1.final")]


def fixtures_a2():
    """Threshold probes for prob, on the scenarios of A1."""
    out = []
    for m in MAX_LENS:
        for start, length in _scenarios(m):
            for T in (2, 3):
                for e in (0, 1):
                    out.append(threshold_probe(f"a2.m{m}.s{start}.l{length}.T{T}.e{e}", m, LO, start, length, T, e))
            out.append(saved_probe(f"a2.saved.m{m}.s{start}.l{length}.eq_lo", m, LO, HI, start, length, 0))
            out.append(saved_probe(f"a2.saved.m{m}.s{start}.l{length}.eq_hi", m, HI, LO, start, length, 0))
            out.append(saved_probe(f"a2.saved.m{m}.s{start}.l{length}.lt_lo", m, LO, HI, start, length, -1))
            out.append(saved_probe(f"a2.saved.m{m}.s{start}.l{length}.gt_hi", m, HI, LO, start, length, +1))
        for mod, length in _final_scenarios(m):
            for T in (2, 3):
                for e in (0, 1):
                    out.append(threshold_probe(f"a2.final.m{m}.n%{mod}.l{length}.T{T}.e{e}", m, LO, None, length, T, e, final_mod=mod))
    return out


A3_MID = 4 * (1 << 20) + 3 * P4 + 5      # pieces 0 .. 1027: the edges between scan threads (4 entries), scan waves (256) and fix-up workgroups (256 pieces)
A3_CARRY = 16 * (1 << 20) + 3 * P4 + 5   # pieces 0 .. 4099: the scan's outer loop carries across 4 096 entries
A3_BIG = (129 << 20) + 4099              # the smallest size at which a wave of the statistics kernel takes a second piece (32 768 waves)


def fixtures_a3_mid():
    """Long runs across pieces 3 -> 4, 255 -> 256 -> 257 and 1023 -> 1024, and runs of max_len -+ 1 that straddle each of those edges."""
    edges = (4 * P4, 256 * P4, 257 * P4, 1024 * P4)
    out = [Fixture("a3.mid.long", compose(A3_MID, [(1, 3 * P4 + 1000, P4 + 500), (2, 255 * P4 + 4000, P4 + 200), (3, 1023 * P4 + 17, P4 + 4000)]))]
    for m in MAX_LENS:
        for d in (-1, +1):
            runs = [(10 + k, e - (m + d) // 2 - k, m + d) for k, e in enumerate(edges)]
            out.append(Fixture(f"a3.mid.m{m}{d:+d}", compose(A3_MID, runs), m))
    return out


def fixtures_a3_carry():
    """One run from piece 4090 into the last piece, and -- another input: the two overlap -- one from piece 2 into piece 4097."""
    return [Fixture("a3.carry.4090_to_last", compose(A3_CARRY, [(1, 4090 * P4 + 123, 9 * P4 - 123 + 2)])),
            Fixture("a3.carry.2_to_4097", compose(A3_CARRY, [(2, 2 * P4 + 9, 4095 * P4 + 300)]))]


def fixture_a3_big():
    """Zero-dominated bytes with about 2 % small values, and a tie probe for either max_len whose run crosses pieces 32767 -> 32769 / 32769 -> 32771 (the
    second pieces of waves 0 .. 2)."""
    rs = np.random.RandomState(129)
    block = np.where(rs.randint(0, 50, (1 << 20) + 37) == 0, rs.randint(1, 5, (1 << 20) + 37), 0).astype(np.uint8)
    d = np.resize(block, A3_BIG)
    at = 32768 * P4
    probes = ((255, 200, 201, at - 255, P4 + 2 * 255), (32, 211, 210, at + 2 * P4 - 32, P4 + 3 * 32))
    lone_at = at + 4 * P4
    for m, x, y, start, length in probes:
        d[start - 1] = 9
        d[start : start + length] = x
        d[start + length] = 9
        for k in range(length // m + 1):                     # y: pcount[x] isolated bytes
            d[lone_at : lone_at + 3] = (9, y, 9)
            lone_at += 2
    d[lone_at] = 9
    return Fixture("a3.big", d)


def fixtures_a4():
    """All 256 symbols in use (the count byte is 0 and 255 symbols are listed), 255 in use, one in use."""
    def spread(symbols, reps):
        seq = []
        for rep in range(reps):
            for s in symbols:
                if rep % 3 < 1 + s % 3:
                    seq += [s] * (1 + (s * 7 + rep) % 5)
        return np.array(seq, dtype=np.uint8)
    return [Fixture("a4.all256", spread(range(256), 3)), Fixture("a4.all256.pieces", spread(range(256), 24)), Fixture("a4.255_without_0", spread(range(1, 256), 3)),
            Fixture("a4.255_without_77", spread([s for s in range(256) if s != 77], 9)), Fixture("a4.one", np.full(2 * P4 + 77, 5, dtype=np.uint8)),
            Fixture("a4.one.byte", np.full(1, 0, dtype=np.uint8))]


A5_SIZE = 3 * G16 + 77


def fixtures_a5():
    """Cut edges of k_le_cuts (a cut: the first token start at or behind every 16 384th byte; inside a flagged run at run start + j max_len, not within the
    input's last 256 bytes).  Piece starts a = 16384 (symbol 60) and 2 * 16384 (symbol 61) in one input."""
    out = []
    for m in MAX_LENS:
        for r in (0, 1, m - 1):                              # (a - run start) % max_len
            for end in (-1, 0, 1, m):                        # the run ends at a + end
                runs = [(LO + k - 1, k * G16 - r - 2 * m, r + 2 * m + end) for k in (1, 2)]
                out.append(Fixture(f"a5.m{m}.r{r}.e{end}.flagged", compose(A5_SIZE, runs), m))
                length = r + 2 * m + end
                singles = _pad_to(length, length // m + 1, 2, 1)[0]     # prob == 2 pcount - 1: the flag stays clear
                out.append(Fixture(f"a5.m{m}.r{r}.e{end}.unflagged", compose(A5_SIZE, runs, [(LO, 1, singles), (HI, 1, singles)]), m))
        a = 2 * G16
        for off in (0, 5):                                   # the first token start at or behind a: g = a + off
            for back in (257, 256, 255):                     # ... which is n - back; the flagged run covers [g - max_len, n)
                n = a + off + back
                out.append(Fixture(f"a5.m{m}.end.g{off}.n-{back}", compose(n, [(LO, a + off - m, n - (a + off - m))]), m))
        out.append(Fixture(f"a5.m{m}.last_piece_without_cut", compose(a + 100, [(LO, a - 3 * m, 100 + 3 * m)]), m))
    out.append(Fixture("a5.all_equal", np.full(A5_SIZE, 5, dtype=np.uint8)))
    return out


def fixtures_small():
    """A1, A2 and A4: the inputs of a few pieces."""
    return fixtures_a1() + fixtures_a2() + fixtures_a4()


LANE_SECTIONS = (131072, 131073)     # from 131 072 sections on the rle8m encoder runs one lane per section


def lane_inputs(seed=5):
    """Inputs for the lane-per-section rle8m encoder: sections of 7 and of 3 bytes (and, with 131 073 sections of the first two, a last section of 131 073
    bytes).  The condition they are chosen for -- the oracle writes a stream for at least two of the cases and refuses at least one -- is asserted in
    tests/test_low_entropy_stats.py."""
    import random

    from hsrle_testlib import mixed_runs

    rng = random.Random(seed)
    return [mixed_runs(rng, 131072 * 7 + 1, alphabet=4), mixed_runs(rng, 131072 * 7 + 1, alphabet=256), mixed_runs(rng, 131072 * 3 + 5, alphabet=2)]
