#!/usr/bin/env python3
"""The segment algebra of the GPU mmtf128 / mmtf256 kernels (hypersonic-rle-kit_amd/csrc/hsrle_mmtf.hip.h), stated on the CPU.

A column of the multi-move-to-front transform is ONE sequential chain over the whole input.  The kernels cut the rows into segments of
R rows and run three passes; this file states each of them in plain Python so that the closed forms can be checked against the sequential
definition before (and without) a kernel:

  pass A  per (segment, column), from the IDENTITY list:
            decode  P: the permutation the segment's ranks apply to the positions of any incoming list   after[i] = before[P[i]]
            encode  (F, K): the list after the segment from identity and the number of distinct symbols; F[:K] are they, most recent first.
                    K is counted without a set: a symbol is new exactly when its rank is >= the number of symbols seen so far.
  pass B  per column, the exclusive scan of the compositions along the segments:
            decode  start[s + 1][i] = start[s][P_s[i]]
            encode  start[s + 1]    = F_s[:K_s] + [x for x in start[s] if x not in F_s[:K_s]]
  pass C  per (segment, column): the sequential step from start[s]; the n % W bytes behind the last row are looked up in the lists as they
          stand after the last row, without an update.

segment_encode / segment_decode give the bytes the reference's mmtf{128,256}_{encode,decode} give (tests/test_mmtf_model.py).
`python tools/mmtf_segment_model.py` runs a self-check against the sequential form.
"""
import random
import sys


def sequential(data, W, decode):
    """The definition (reference: src/mmtf.c): one pass, W lists."""
    n = len(data)
    rows = n // W
    out = bytearray(n)
    lists = [list(range(256)) for _ in range(W)]
    for i in range(rows * W):
        l = lists[i % W]
        if decode:
            k = data[i]
            out[i] = l[k]
        else:
            k = l.index(data[i])
            out[i] = k
        l.insert(0, l.pop(k))
    for i in range(rows * W, n):
        l = lists[i - rows * W]
        out[i] = l[data[i]] if decode else l.index(data[i])
    return bytes(out)


def _column(data, W, c, first_row, rows):
    return [data[(first_row + r) * W + c] for r in range(rows)]


def pass_a_decode(ranks):
    """P with after[i] = before[P[i]]: the MTF of the ranks run on position ids."""
    p = list(range(256))
    for k in ranks:
        p.insert(0, p.pop(k))
    return p


def pass_a_encode(symbols):
    """(F, K): the list after the symbols from identity, and how many distinct ones there were."""
    f = list(range(256))
    k_seen = 0
    for x in symbols:
        k = f.index(x)
        if k >= k_seen:          # unseen symbols stay behind the seen ones, in identity order
            k_seen += 1
        f.insert(0, f.pop(k))
    return f, k_seen


def compose_decode(before, p):
    return [before[p[i]] for i in range(256)]


def compose_encode(before, f, k):
    head = f[:k]
    member = set(head)
    return head + [x for x in before if x not in member]


def segment_transform(data, W, segment_rows, decode):
    n = len(data)
    rows = n // W
    R = max(1, int(segment_rows))
    S = (rows + R - 1) // R
    out = bytearray(n)
    final = [list(range(256)) for _ in range(W)]
    for c in range(W):
        # pass A (the last segment needs no state)
        states = []
        for s in range(max(S - 1, 0)):
            col = _column(data, W, c, s * R, min(R, rows - s * R))
            states.append(pass_a_decode(col) if decode else pass_a_encode(col))
        # pass B
        start = [list(range(256))]
        for s in range(max(S - 1, 0)):
            start.append(compose_decode(start[s], states[s]) if decode else compose_encode(start[s], *states[s]))
        # pass C
        for s in range(S):
            l = list(start[s])
            for r in range(s * R, min((s + 1) * R, rows)):
                i = r * W + c
                if decode:
                    k = data[i]
                    out[i] = l[k]
                else:
                    k = l.index(data[i])
                    out[i] = k
                l.insert(0, l.pop(k))
            if s == S - 1:
                final[c] = l
    for i in range(rows * W, n):
        l = final[i - rows * W]
        out[i] = l[data[i]] if decode else l.index(data[i])
    return bytes(out)


def segment_encode(data, W, segment_rows):
    return segment_transform(data, W, segment_rows, False)


def segment_decode(data, W, segment_rows):
    return segment_transform(data, W, segment_rows, True)


def main():
    rng = random.Random(5)
    checked = 0
    for W in (16, 32):
        for R in (1, 2, 7, 64):
            for n in (0, 1, W - 1, W, W + 1, 64 * W + 5, 3001):
                for alphabet in (1, 2, 5, 256):
                    data = bytes(rng.randrange(alphabet) for _ in range(n))
                    for decode in (False, True):
                        if segment_transform(data, W, R, decode) != sequential(data, W, decode):
                            print(f"MISMATCH W={W} R={R} n={n} alphabet={alphabet} decode={decode}")
                            return 1
                        checked += 1
    print(f"mmtf segment model: {checked} cases equal to the sequential form")
    return 0


if __name__ == "__main__":
    sys.exit(main())
