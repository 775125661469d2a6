"""Container inputs whose LAST block ends just behind (or on, or just in front of) a 4 KiB window edge -- a helper module, no test and no GPU.

The windowed encoders (csrc/hsrle_encode8pw.hip.h, hsrle_encodeSpw.hip.h, hsrle_encodeLpw.hip.h) walk a block in windows of 4 KiB: one wave per block sizes it, one
wave per WINDOW writes it.  A run belongs to the window in which its match stretch ends, and that is up to S bytes in front of the run's end: a block that ends
1 .. S - 1 bytes into a window on a run has that run stored by the window in front, and the last window has to know that the stream ended on a run (the short
terminator) from what the window in front hands over.  Block sizes are multiples of 128, so only a container's short last block can end there.

A case is two full blocks of B bytes and a last block of L = 4096 k + r bytes, r = -1 .. S + 1, whose end is one of SHAPES (ISSUE: what the last window's
terminator and its trailing literals can look like).  cases(codec) -> [(name, B, data)]; case_list(codec) -> the same with the parameters as fields.
"""
import collections
import random

import numpy as np

from hsrle_testlib import CODEC_BY_KEY
from test_gpu_pp import KEYS, WINDOWED_L_KEYS, WINDOWED_S_KEYS, _periodic

WINDOW = 4096
ALL_KEYS = KEYS + WINDOWED_S_KEYS + WINDOWED_L_KEYS                  # every codec whose blocks above 4 KiB are walked in windows
BLOCKS_AND_WINDOWS = [(8192, 1), (12416, 1), (12416, 2), (12416, 3), (65536, 15)]
SHAPES = ("to_end", "to_end_long", "short_of_end", "whole", "fuzzer", "fuzzer_whole", "literals", "short_run_to_end")
REPRESENTATIVE_KEYS = ["rle16_sym_packed", "rle32_byte", "rle64_3symlut_byte_short", "rle24_1symlut_sym_short", "rle16_7symlut_sym", "rle48_7symlut_byte_short"]

# name: "B=.. k=.. r=.. <shape>[ t=..][ run=..] <equal|distinct>"; t: short_of_end's distance to the end, run: short_run_to_end's length; sym: "" for `literals`
Case = collections.namedtuple("Case", "name B data k r shape t sym")


def remainders(S):
    return list(range(-1, S + 2))


def run_length(S):
    """R: whole symbols, long enough that every codec stores the run whatever lies in front of it"""
    return S * ((3 * S + 20) // S)


_FULL, _RANDOM, _LITERALS = {}, {}, {}


def full_blocks(B):
    """the two full blocks in front: the `periods` data of test_gpu_pp's wide cases (runs of many periods and lengths between literal stretches)"""
    if B not in _FULL:
        rng = np.random.default_rng(7051 + B)
        _FULL[B] = _periodic(rng, 2 * B, [1, 2, 3, 4, 6, 8, 12, 16], 256, 40, [4, 5, 6, 7, 8, 9, 11, 12, 13, 16, 17, 18, 19, 23, 24, 25, 40, 64, 100, 300, 2000, 9000])
        _FULL[B].setflags(write=False)
    return _FULL[B]


def _random_block(k, L):
    if k not in _RANDOM:
        _RANDOM[k] = np.random.default_rng(4096 + k).integers(0, 256, WINDOW * k + 32, dtype=np.uint8)
    return _RANDOM[k][:L].copy()


def _no_run_bytes(S, n):
    """n bytes of which none equals the byte 1, S or 2 S positions in front of it: no run of any codec of symbol width S (or 1)"""
    if S not in _LITERALS:
        rng = random.Random(9000 + S)
        seq = bytearray()
        for i in range(2 * WINDOW + 32):
            v = rng.randrange(256)
            while any(i >= d and seq[i - d] == v for d in (1, S, 2 * S)):
                v = (v + 1) & 255
            seq.append(v)
        _LITERALS[S] = np.frombuffer(bytes(seq), dtype=np.uint8)
    return _LITERALS[S][:n]


def _fill(sym, n, phase=0):
    """n bytes of the symbol's repetitions, starting `phase` bytes into it"""
    return np.resize(np.roll(sym, -phase), n) if n else np.empty(0, dtype=np.uint8)


def _put_run(blk, sym, start, end):
    """sym repeated over blk[start:end]; the byte in front does not continue it backwards (it differs from the byte S positions behind it, sym[-1])"""
    blk[start:end] = _fill(sym, end - start)
    if start > 0 and blk[start - 1] == sym[-1]:
        blk[start - 1] ^= 0x5A


def _last_blocks(S, k, r, rng):
    """(shape, t, symbol kind, last block) for one block length"""
    L = WINDOW * k + r
    R = run_length(S)
    equal = np.full(S, rng.integers(0, 256), dtype=np.uint8)
    distinct = rng.permutation(256)[:S].astype(np.uint8)
    for kind, sym in (("equal", equal), ("distinct", distinct)):
        blk = _random_block(k, L)
        _put_run(blk, sym, L - R, L)
        yield "to_end", 0, kind, blk

        blk = _random_block(k, L)
        # (4096 + R bytes, for 3 and 6 byte symbols the next whole symbol: the run has to END on one; a last block of one window: it starts behind the first bytes)
        _put_run(blk, sym, L - min((WINDOW + R + S - 1) // S * S, (L - 1) // S * S), L)
        yield "to_end_long", 0, kind, blk

        for t in range(1, S + 1):
            blk = _random_block(k, L)
            start = L - t - R
            _put_run(blk, sym, start, L - t)
            blk[L - t :] = _fill(sym, t, (L - t - start) % S) ^ 0x5A            # none of the t bytes behind the run continues it
            yield "short_of_end", t, kind, blk

        yield "whole", 0, kind, _fill(sym, L)

        head = np.array([rng.integers(0, 256), sym[0], rng.integers(0, 256), sym[0], rng.integers(0, 256)], dtype=np.uint8)
        yield "fuzzer", 0, kind, np.concatenate([head, _fill(sym, L - 5)])
        pad = (L - 5) % S
        if pad:                                                               # (no pad: `fuzzer` already ends on a whole symbol)
            yield "fuzzer_whole", 0, kind, np.concatenate([head, np.zeros(pad, dtype=np.uint8), _fill(sym, L - 5 - pad)])

        for run in (2 * S, 3 * S):                                            # below / at the store thresholds: the oracle says which terminator follows
            blk = _random_block(k, L)
            _put_run(blk, sym, L - run, L)
            yield "short_run_to_end", run, kind, blk

    blk = _random_block(k, L)
    W = min(L, 2 * WINDOW + r)
    blk[L - W :] = _no_run_bytes(S, W)
    yield "literals", 0, "", blk


def case_list(codec, blocks_and_windows=BLOCKS_AND_WINDOWS):
    """the cases of one codec (a Codec of hsrle_testlib or its key), in a fixed order"""
    codec = CODEC_BY_KEY[codec] if isinstance(codec, str) else codec
    S = codec.S
    rng = np.random.default_rng(8800 + S)
    for B, k in blocks_and_windows:
        front = full_blocks(B)
        for r in remainders(S):
            for shape, t, kind, blk in _last_blocks(S, k, r, rng):
                assert blk.size == WINDOW * k + r and blk.dtype == np.uint8
                extra = f" t={t}" if shape == "short_of_end" else (f" run={t}" if shape == "short_run_to_end" else "")
                name = f"B={B} k={k} r={r} {shape}{extra}{' ' + kind if kind else ''}"
                yield Case(name, B, np.concatenate([front, blk]), k, r, shape, t, kind)


def cases(codec):
    return [(c.name, c.B, c.data) for c in case_list(codec)]


def summary(names):
    """case names folded for a failure message: per shape, how many of them at which r"""
    by_shape = collections.OrderedDict()
    for n in names:
        f = n.split()
        shape, r = f[3], int(f[2][2:])
        by_shape.setdefault(shape, collections.Counter())[r] += 1
    return "; ".join(f"{s}: " + ", ".join(f"r={r} x{c}" for r, c in sorted(cnt.items())) for s, cnt in by_shape.items())
