"""Heterogeneous decoder inputs, built on the host (a helper module, not a conftest).

The GPU decode tests elsewhere feed the block decoders containers the GPU encoders just wrote, from data that is roughly uniform across
blocks.  Here every block is one of five kinds, the mixture of each wave of 64 consecutive blocks (= one workgroup of k_decode_blocks, a lane
per block) is fixed by construction, the block streams come from the CPU oracle and the container from hsrle_testlib.build_container -- so the
container's ratio, and with it the stream ring the plain decode takes (hsrle.decode_ring), is a property of the fixture, not of an encoder run.

Block kinds, for a codec of S-byte symbols and blocks of B bytes:
  Z  the whole block is one S-byte symbol                                       (one packet: the lane is done after its first trip)
  L  random bytes                                                               (literal only: the lane that needs the most stream bytes)
  D  three S-byte symbols in rotation, R .. R + 2 repeats each, back to back    (the densest packet chain; listed symbols keep returning)
  M  runs of R / R + 1 / R + 3 / R + 7 repeats of three symbols, 0 - 3 literal bytes between
  Both start with one run of R + 6 repeats of each symbol.  R = 2 (2 - 4 repeats; 2 / 3 / 5 / 9) for the codecs whose encoders store such runs, else the shortest run they do store: dense_repeats().  The Single codecs store
  runs of one symbol per block, so in their D blocks the other two symbols of the rotation come once each.  For every codec of 8 bit symbols a D block has more
  packets than a packet list holds (B / 8 + 2 entries).
  V  the oracle's video-shaped synthetic data for S
Layouts, per wave of 64 blocks, shuffled with a fixed seed per codec:
  sparse  3 L, 3 D, 3 M, 8 V, 47 Z   -- ratio <= 0.18: below every small-ring threshold (0.215 / 0.25), a few lanes that need both passes and
                                        the top-up beside neighbours that finish after one packet
  dense   24 L, 12 D, 12 M, 8 V, 8 Z -- ratio >= 0.40: the 128-byte ring
A container's trailing PARTIAL wave (the 70-block container of 16 KiB blocks has one of six blocks) is the start of another shuffle: the mixture is
promised for full waves only.  The last block is partial and ends off a 16-byte boundary.  tests/test_decoder_fixtures.py asserts these properties for all 110 codecs on the CPU.
Sparse containers are not built below B = 2048: at 1024 the ratio reaches 0.21 (the blocks' headers and terminators weigh more).
"""
import collections
import random

import numpy as np

from hsrle_testlib import CODECS, PACKED_SINGLE, SINGLE, SINGLE_SHORT, SYNTH_VIDEO, Oracle, build_container

LAYOUTS = {"sparse": (("L", 3), ("D", 3), ("M", 3), ("V", 8), ("Z", 47)),
           "dense": (("L", 24), ("D", 12), ("M", 12), ("V", 8), ("Z", 8))}
WAVE = 64
SPARSE_MIN_BLOCK = 2048
PRIME = 6                          # the first run of each symbol of a D / M block: R + PRIME repeats
TAIL_PAD = 32                      # include/hsrle.h: HSRLE_CONTAINER_TAIL_PAD

Fixture = collections.namedtuple("Fixture", "codec layout B data kinds streams container U payload_size ratio")

_ORACLE = None


def oracle_instance():
    global _ORACLE
    if _ORACLE is None:
        _ORACLE = Oracle()
    return _ORACLE


def _symbols(rng, S, n=3):
    """n different S-byte symbols, none of them periodic in itself for S > 1 (its bytes are not all equal)."""
    out = []
    while len(out) < n:
        s = bytes(rng.randrange(256) for _ in range(S))
        if s not in out and (S == 1 or len(set(s)) > 1):
            out.append(s)
    return out


def _is_single(codec):
    return codec.family in (SINGLE, PACKED_SINGLE, SINGLE_SHORT)


def block_bytes(kind, codec, B, rng, video=None, R=None):
    """One block of `kind` (B bytes).  V takes its bytes from `video` (B bytes of the oracle's synth); R: dense_repeats(codec)."""
    S = codec.S
    if kind == "Z":
        return (_symbols(rng, S, 1)[0] * (B // S + 1))[:B]
    if kind == "L":
        return np.random.RandomState(rng.randrange(1 << 31)).randint(0, 256, B, dtype=np.uint8).tobytes()
    if kind == "V":
        assert video is not None and len(video) == B
        return bytes(video)
    R = dense_repeats(codec) if R is None else R
    syms = _symbols(rng, S)
    # (the first run of each symbol is long: a list codec stores a short run only of a symbol it has listed, and a Short encoder that has stored nothing for a while
    #  pays for a long literal range with every packet and then never starts -- such a block would be one more literal-only block)
    out = bytearray(b"".join(sym * (R + PRIME) for sym in syms))
    k = rng.randrange(3)
    while len(out) < B:
        if kind == "D":
            # (the Single codecs store runs of ONE symbol per block: the other two of the rotation come once each, so a packet still is a few bytes)
            out += syms[k] * (1 if _is_single(codec) and k != 0 else rng.choice((R, R + 1, R + 2)))
            k = (k + 1) % 3
        else:
            assert kind == "M"
            out += syms[rng.randrange(3)] * rng.choice((R, R + 1, R + 3, R + 7))
            out += bytes(rng.randrange(256) for _ in range(rng.randrange(4)))
    return bytes(out[:B])


_REPEATS = {}


def dense_repeats(codec):
    """R: the shortest run, in symbols, of the D and M blocks of this codec.  The recipe says 2 (D: 2 - 4 repeats, M: 2 / 3 / 5 / 9) and that is what most codecs
    get -- but an encoder that leaves such runs as literals (rle8_multi stores runs from 6 bytes on, rle8_packed_multi and rle8_single from 4, most other 8 bit
    codecs and the plain / Packed 16 and sym 24 bit ones from 3 symbols) would make D one more literal-only block.  So R is the smallest count for which the
    oracle's encoder stores EVERY run of a 4 KiB probe block of R .. R + 2 repeats (D: R .. R + 2, M: R / R + 1 / R + 3 / R + 7)."""
    if codec.key not in _REPEATS:
        for R in range(2, 17):
            block = block_bytes("D", codec, 4096, random.Random(5), R=R)
            packets = oracle_instance().run_packets(codec, oracle_instance().compress_blocks(codec, np.frombuffer(block, dtype=np.uint8), 4096)[0], 4096)
            if packets >= dense_packets_min(codec, 4096, R):
                break
        else:
            raise AssertionError(f"{codec.key}: no run length up to 18 symbols makes a packet-dense block")
        _REPEATS[codec.key] = R
    return _REPEATS[codec.key]


def dense_packets_min(codec, n, R=None):
    """The fewest run packets of n bytes of a D block in which every run is stored: a run (Single: with the two bytes between runs) is at most this long."""
    R = dense_repeats(codec) if R is None else R
    return max(n // ((R + 2) * codec.S + (2 if _is_single(codec) else 0)) - 2 * PRIME, 0)   # (- the room of the three long first runs)


def wave_kinds(layout, rng):
    kinds = [k for k, n in LAYOUTS[layout] for _ in range(n)]
    assert len(kinds) == WAVE
    rng.shuffle(kinds)
    return kinds


def default_shape(B):
    """(blocks, bytes of the last block): three waves of 4 KiB blocks, 70 blocks of 16 KiB (~1.1 MiB: the largest container); the last block is
    partial and ends off a 16-byte boundary."""
    return (70 if B > 4096 else 3 * WAVE), B // 2 + 5


def _seed(codec, layout, B):
    return 1000003 * CODECS.index(codec) + 101 * B + (7 if layout == "dense" else 0)


def _video(codec, count, B):
    return oracle_instance().synth(SYNTH_VIDEO, codec.S, 11 + CODECS.index(codec), max(count, 1) * B)


def _front(codec, layout, B, blocks):
    """The kinds of all `blocks` blocks as the shuffle leaves them, and the bytes of all but the last."""
    assert layout in LAYOUTS and (layout != "sparse" or B >= SPARSE_MIN_BLOCK), "sparse containers are not built below 2048-byte blocks"
    rng = random.Random(_seed(codec, layout, B))
    kinds = []
    while len(kinds) < blocks:
        kinds += wave_kinds(layout, rng)
    kinds = kinds[:blocks]
    video = _video(codec, kinds.count("V"), B)
    parts, v = [], 0
    for kind in kinds[:-1]:
        parts.append(block_bytes(kind, codec, B, rng, video[v * B : (v + 1) * B] if kind == "V" else None))
        v += kind == "V"
    return kinds, parts


def _last(codec, layout, B, blocks, kind, last_len):
    """The last block: drawn from a generator of its own, so the blocks in front of it are what they are whatever its kind and length."""
    rng = random.Random(_seed(codec, layout, B) + 977 * blocks + 31 * "ZLDMV".index(kind))
    return block_bytes(kind, codec, B, rng, _video(codec, 1, B)[:B] if kind == "V" else None)[:last_len]


def build_input(codec, layout, B, blocks=None, last_len=None, last_kind=None):
    """(bytes as a numpy uint8 array, kind of every block).  Deterministic per (codec, layout, B, blocks, last_len, last_kind)."""
    if blocks is None:
        blocks, dflt = default_shape(B)
        last_len = dflt if last_len is None else last_len
    assert 1 <= last_len <= B
    kinds, parts = _front(codec, layout, B, blocks)
    if last_kind is not None:
        kinds[-1] = last_kind
    parts.append(_last(codec, layout, B, blocks, kinds[-1], last_len))
    return np.frombuffer(b"".join(parts), dtype=np.uint8), kinds


def tail_matrix(codec, layout, B, blocks, lengths, last_kinds="LZD"):
    """The fixtures fixture(codec, layout, B, blocks, n, k) for n in lengths, k in last_kinds -- with the blocks in front of the last one generated and
    encoded once (they are the same in all of them)."""
    ora = oracle_instance()
    kinds, parts = _front(codec, layout, B, blocks)
    front = np.frombuffer(b"".join(parts), dtype=np.uint8)
    front_streams = ora.compress_blocks(codec, front, B) if blocks > 1 else []
    for k in last_kinds:
        for n in lengths:
            last = np.frombuffer(_last(codec, layout, B, blocks, k, n), dtype=np.uint8)
            yield assemble(codec, layout, B, np.concatenate((front, last)), kinds[:-1] + [k], front_streams + ora.compress_blocks(codec, last, B))


def assemble(codec, layout, B, data, kinds, streams, codec_index=None):
    payload = sum(len(s) for s in streams)
    container = build_container(CODECS.index(codec) if codec_index is None else codec_index, data.size, B, streams)
    return Fixture(codec, layout, B, data, kinds, streams, container, data.size, payload, (payload + TAIL_PAD) / data.size)


_CACHE = collections.OrderedDict()
_CACHE_MAX = 12          # (a fixture is ~2.5 MiB; the tests of one codec run back to back, so a few entries serve)


def fixture(codec, layout, B, blocks=None, last_len=None, last_kind=None):
    """The input, the oracle's block streams and the host-built container, cached per arguments."""
    key = (codec.key, layout, B, blocks, last_len, last_kind)
    if key in _CACHE:
        _CACHE.move_to_end(key)
        return _CACHE[key]
    data, kinds = build_input(codec, layout, B, blocks, last_len, last_kind)
    f = assemble(codec, layout, B, data, kinds, oracle_instance().compress_blocks(codec, data, B))
    _CACHE[key] = f
    while len(_CACHE) > _CACHE_MAX:
        _CACHE.popitem(last=False)
    return f


def expected_ring(fix):
    """What hsrle.decode_ring must say for this fixture -- the tests assert it, so each of them names the kernel it ran."""
    if fix.codec.S >= 6 or fix.layout == "dense":
        return 128
    return 64


def blocks_of_kind(fix, kind):
    return [i for i, k in enumerate(fix.kinds) if k == kind]
