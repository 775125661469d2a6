"""The inputs of tests/block_end_cases.py do what they are for (no GPU): the oracle's streams of every case are streams of the codec's grammar that give the
input back, the last block's terminator is the one the shape was built for -- `to_end` / `to_end_long` end on a stored run (the short "ended" terminator),
`short_of_end` on t literal bytes that begin in the window in FRONT of the last one where t > r -- every case takes the windowed encoder, and the compiled
reference (where it was built) writes the very same last streams and reads them back."""
import os

import pytest

import block_end_cases as BE
import stream_grammar as SG
from hsrle_testlib import CODEC_BY_KEY

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "hypersonic-rle-kit_amd", "libhsrle_hip.so")
PATH_POSITION_PARALLEL = 3


def test_keys_and_case_names():
    assert len(BE.ALL_KEYS) == 86 and len(set(BE.ALL_KEYS)) == 86
    assert set(BE.REPRESENTATIVE_KEYS) <= set(BE.ALL_KEYS)
    for key in ("rle8_multi", "rle24_sym", "rle64_7symlut_byte_short"):
        S = CODEC_BY_KEY[key].S
        got = BE.cases(key)
        names = [n for n, _, _ in got]
        assert len(set(names)) == len(names)
        for B, k in BE.BLOCKS_AND_WINDOWS:
            for r in BE.remainders(S):
                here = [n for n in names if n.startswith(f"B={B} k={k} r={r} ")]
                assert {n.split()[3] for n in here} >= set(BE.SHAPES) - {"fuzzer_whole"}, (key, B, k, r)          # never an r or a shape less
                assert {n for n in here if " short_of_end " in n} == {f"B={B} k={k} r={r} short_of_end t={t} {s}" for t in range(1, S + 1) for s in ("equal", "distinct")}
        assert all(d.size == 2 * B + BE.WINDOW * int(n.split()[1][2:]) + int(n.split()[2][2:]) for n, B, d in got)
        assert BE.cases(key)[-1][2].tobytes() == got[-1][2].tobytes()                                                # the same bytes every time
    names = ["B=8192 k=1 r=1 to_end equal", "B=8192 k=1 r=2 to_end distinct", "B=12416 k=2 r=1 to_end equal", "B=8192 k=1 r=-1 short_of_end t=2 equal"]
    assert BE.summary(names) == "to_end: r=1 x2, r=2 x1; short_of_end: r=-1 x1"


def _terminator(forms):
    """the one terminator form of a parsed stream (term.lit.zero only says that a literal terminator had no literals)"""
    terms = [f for f in forms if f.startswith("term.") and f != "term.lit.zero"]
    assert len(terms) == 1 and forms[terms[0]] == 1, terms
    return terms[0]


def _encode_path(key):
    """hsrle_encode_path of the HIP library for this codec (a host function: no device needed), or None where the library is not built"""
    if not os.path.exists(LIB):
        return None
    import hsrle

    cid = hsrle.codec_id(key)
    return lambda U, B: hsrle.lib().hsrle_encode_path(cid, U, B)


@pytest.mark.parametrize("key", BE.ALL_KEYS)
def test_cases_end_as_their_shape_says(oracle, key):
    codec = CODEC_BY_KEY[key]
    g = SG.grammar(codec)
    path = _encode_path(key)
    checked_front = set()
    ended = literal = in_front = 0
    for c in BE.case_list(codec):
        B = c.B
        what = f"{key} {c.name}"
        if path is not None:
            assert path(c.data.size, B) == PATH_POSITION_PARALLEL, what
        if B not in checked_front:                                              # (the two full blocks are the same in every case of this block size)
            checked_front.add(B)
            for i, s in enumerate(oracle.compress_blocks(codec, c.data[: 2 * B], B)):
                assert SG.parse(g, s)[0] == c.data[i * B : (i + 1) * B].tobytes(), f"{what}: block {i}"
        last = c.data[2 * B :]
        (stream,) = oracle.compress_blocks(codec, last, B)
        out, forms, headers = SG.parse(g, stream)
        assert out == last.tobytes(), what
        term = _terminator(forms)
        at, hl = headers[-1]
        trailing = len(stream) - at - hl
        last_window = last.size - (last.size - 1) // BE.WINDOW * BE.WINDOW      # the bytes of the last window
        if c.shape in ("to_end", "to_end_long"):
            assert term.endswith("end"), f"{what}: {term}"
        if c.shape == "short_of_end":
            assert not term.endswith("end") and trailing == c.t, f"{what}: {term}, {trailing} trailing literals"
        if term.endswith("end"):
            ended += 1
            assert trailing == 0, what
        else:
            literal += 1
            in_front += trailing > last_window
    assert ended and literal, f"{key}: {ended} ended, {literal} literal terminators"
    assert in_front, f"{key}: no last block whose trailing literals begin in front of its last window"


@pytest.mark.parametrize("key", BE.ALL_KEYS)
def test_the_reference_writes_the_same_last_blocks(reference, oracle, key):
    """(skipped where the compiled reference is absent)"""
    codec = CODEC_BY_KEY[key]
    for c in BE.case_list(codec):
        last = c.data[2 * c.B :]
        (stream,) = oracle.compress_blocks(codec, last, c.B)
        ref = reference.compress(codec, last.tobytes())
        assert ref == stream, f"{key} {c.name}: the reference's stream of the last block differs from the oracle's"
        assert reference.decompress(codec, ref) == last.tobytes(), f"{key} {c.name}"
