"""The CPU twin of test_gpu_decode_loop_order.py: the containers of decode_loop_order_fixtures.py are what they claim to be.

Every stream decodes under the oracle's decoder to the bytes its writer intended (and under the compiled reference, where that is built); every named block kind
occurs in every wave -- read from where the packets LIE, not from the labels; every terminator form without literals stands behind a last packet that ends on a
step boundary at least once per codec and mixture; the sparse containers stay below the 64-byte ring's threshold, the dense ones above the 128-byte ring's; the
malformed streams are refused by the oracle and have a recorded parent verdict for every decode variant."""
import json
import os
import random

import numpy as np
import pytest

import decode_loop_order_fixtures as L
import decoder_fixtures as F
import stream_grammar as G
from hsrle_testlib import REPO, Reference

GOLDEN = os.path.join(REPO, "tests", "golden", "decode_loop_order_status.json")
VARIANTS = ("plain", "windowed", "entries")
CASES = [(c, m) for c in L.CODECS8 for m in L.MIXTURES]


def test_the_codecs_are_the_one_byte_symbol_ids():
    assert [c.key for c in L.CODECS8] == ["rle8_multi", "rle8_packed_multi", "rle8_3symlut", "rle8_7symlut", "rle8_single", "rle8_packed_single", "rle8_multi_short",
                                          "rle8_1symlut_short", "rle8_3symlut_short", "rle8_7symlut_short", "rle8_single_short"]


@pytest.mark.parametrize("codec, mixture", CASES, ids=lambda v: getattr(v, "key", v))
def test_streams_decode_and_every_kind_is_there(codec, mixture):
    ora = F.oracle_instance()
    ref = Reference() if Reference.available() else None
    g = G.grammar(codec)
    forms_seen = set()
    for B, blocks in L.SHAPES:
        fix, blks = L.container(codec, mixture, B, blocks)
        what = f"{codec.key} {mixture} B {B} x {blocks}"
        assert fix.U == B * blocks and len(blks) == blocks
        assert (fix.ratio <= 0.18) if mixture == "sparse" else (fix.ratio >= 0.40), f"{what}: ratio {fix.ratio:.3f}"
        assert F.expected_ring(fix) == (64 if mixture == "sparse" else 128)
        wave = set()
        for i, blk in enumerate(blks):
            want = bytes(fix.data[i * B : (i + 1) * B])
            assert blk.out == want and G.parse(g, blk.stream)[0] == want, f"{what}: block {i} ({blk.kind}) is not a stream of its grammar"
            assert ora.decompress(codec, blk.stream, B) == want, f"{what}: the oracle decodes block {i} ({blk.kind}) to other bytes"
            if ref is not None:
                assert ref.decompress(codec, blk.stream, B) == want, f"{what}: the compiled reference decodes block {i} ({blk.kind}) to other bytes"
            have = L.properties(blk, B)
            label = "Lt" if (blk.kind == "L127" and B == 256) else blk.kind
            assert label in have, f"{what}: block {i} is labelled {blk.kind} and has {sorted(have)}"
            if i < F.WAVE:
                wave |= have
            if blk.kind == "T":
                forms_seen.add((blk.term.end, blk.term.cw, blk.term.rw))
        need = set(L.KINDS) - ({"L127"} if B == 256 else set()) | ({"Lt"} if B == 256 else set())
        assert need <= wave, f"{what}: the full wave lacks {sorted(need - wave)}"
        assert sum(1 for b in blks[: F.WAVE] if b.kind == "I") >= 4, f"{what}: no idle neighbours"
    assert forms_seen == set(L.last_forms(g)), f"{codec.key} {mixture}: terminator forms behind a last packet on a step boundary: {sorted(forms_seen)}"


@pytest.mark.parametrize("codec", L.CODECS8, ids=lambda c: c.key)
def test_malformed_streams(codec):
    ora = F.oracle_instance()
    golden = json.load(open(GOLDEN))
    for B in L.BLOCK_SIZES:
        for what in L.malformed_kinds(codec):
            stream, front = L.malformed_stream(codec, what, B, random.Random(1))
            assert int.from_bytes(stream[4:8], "little") == len(stream) and int.from_bytes(stream[:4], "little") == B, "the stream header is consistent"
            assert len(front) == (B if what == "no_terminator" else 63 + (40 if what == "cut_literal" else 0))
            assert ora.decompress(codec, stream, B) is None, f"{codec.key} B {B}: the oracle accepts the stream `{what}`"
            for variant in VARIANTS:
                assert L.golden_key(codec, what, variant) in golden, "no recorded parent verdict"
            for mixture in L.MIXTURES:
                for blocks in L.BLOCK_COUNTS:
                    fix = L.malformed_container(codec, mixture, B, blocks, what)
                    assert fix.streams[L.VICTIM] != L.container(codec, mixture, B, blocks)[0].streams[L.VICTIM]


def test_window_ranges_lie_inside():
    fix, _ = L.container(L.CODECS8[0], "sparse", 256, 64)
    for off, n in L.window_ranges(fix) + [L.victim_window(fix)]:
        assert 0 <= off and n > 0 and off + n <= fix.U and (off != 0 or n != fix.U)
    assert np.array_equal(fix.data, np.frombuffer(b"".join(b.out for b in L.container(L.CODECS8[0], "sparse", 256, 64)[1]), dtype=np.uint8))
