"""The 8 bit packet loop of k_decode_blocks on streams whose packets are PLACED against its 128-byte steps (tests/decode_loop_order_fixtures.py): runs and
literal stretches that cross a step boundary by 1, 15, 16, 17 and 127 bytes, a run over a whole step, a literal stretch no ring holds, packets and last packets
that end exactly on a boundary with every terminator form behind them, header chains that straddle the end of the resident ring bytes, a packet every few bytes --
all of them in every wave, beside neighbours that are done after one packet.  These are the lanes for which the ORDER of the loop's three sections (header,
literals, run; hsrle_codecs.h: dec8_loop_lrh) decides in which trip they parse; the bytes must not depend on it.

Every codec id of one-byte symbols; blocks of 256 and 384 bytes (two and three steps); 64 and 65 blocks; a sparse mixture (the 64-byte ring) and a dense one (the
128-byte ring); the plain decode, the windowed decode and the decode from entry records (one lane per 128 bytes).  The expected bytes are the oracle decoder's
(tests/test_decode_loop_order_fixtures.py proves them equal to the writers' intended output, which is what is compared here).  The malformed containers must end
with exactly the status the parent of the loop-order change reported for them (tests/golden/decode_loop_order_status.json, recorded once from the parent's build
with record_verdicts below), and with the guards around the output untouched.  The helpers are those of test_gpu_decode_variants.py."""
import json
import os

import numpy as np
import pytest

import decode_loop_order_fixtures as L
from hsrle_testlib import REPO
from test_gpu_decode_variants import Arena, _check_blocks, _named_ring, _status, _upload, hs  # noqa: F401  (hs: the module's fixture)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(REPO, "tests", "golden", "decode_loop_order_status.json")
VARIANTS = ("plain", "windowed", "entries")
CASES = [(c, m) for c in L.CODECS8 for m in L.MIXTURES]


def _workspace(hs, info):
    import torch

    return torch.full((max(hs.split_workspace_size(info, None, L.SUB_BLOCK), 16),), 0xC3, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("codec, mixture", CASES, ids=lambda v: getattr(v, "key", v))
def test_placed_packets(hs, codec, mixture):
    import torch

    for B, blocks in L.SHAPES:
        fix, _ = L.container(codec, mixture, B, blocks)
        what = f"{codec.key} {mixture} B {B} x {blocks}"
        ring = _named_ring(hs, fix, what)
        assert ring == (64 if mixture == "sparse" else 128)
        container, info = _upload(hs, fix)
        assert info.blockCount == blocks
        arena, status = Arena(fix.U), _status()
        for first, count in ((0, blocks),) + (((63, 2), (64, 1)) if blocks == 65 else ((63, 1),)):
            arena.reset()
            hs.decompress_async(container, info, arena.view, status, first_block=first, block_count=count)
            _check_blocks(fix, arena, status, first, count, f"{what} ring {ring} blocks [{first}, +{count})")
        arena.reset()
        hs.decompress_split_async(container, info, arena.view, _workspace(hs, info), status, sub_block=L.SUB_BLOCK)
        _check_blocks(fix, arena, status, 0, blocks, f"{what} from entry records at every {L.SUB_BLOCK} bytes")
        runs = []
        for off, n in L.window_ranges(fix):
            a, st = Arena(n), torch.zeros(4, dtype=torch.uint8, device="cuda")
            hs.decompress_range_dev_async(container, info, off, n, a.view, st)
            runs.append((off, n, a, st))
        torch.cuda.synchronize()
        for off, n, a, st in runs:
            w = f"{what} window [{off}, +{n})"
            assert int.from_bytes(st.cpu().numpy().tobytes(), "little") == hs.MONO_DONE == 0, f"{w}: status"
            out, guards = a.host()
            assert np.array_equal(out, fix.data[off : off + n]), f"{w}: differs from the intended bytes"
            assert guards, f"{w}: bytes outside the output were written"


def verdict(hs, fix, variant):
    """(status word, guards untouched, the output bytes and the offset of their first byte) of one decode variant of a container with a malformed block"""
    import torch

    container, info = _upload(hs, fix)
    if variant == "windowed":
        off, n = L.victim_window(fix)
        arena, st = Arena(n), torch.zeros(4, dtype=torch.uint8, device="cuda")
        hs.decompress_range_dev_async(container, info, off, n, arena.view, st)
        torch.cuda.synchronize()
        word = int.from_bytes(st.cpu().numpy().tobytes(), "little")
    else:
        off, arena, st = 0, Arena(fix.U), _status()
        if variant == "plain":
            hs.decompress_async(container, info, arena.view, st)
        else:
            hs.decompress_split_async(container, info, arena.view, _workspace(hs, info), st, sub_block=L.SUB_BLOCK)
        torch.cuda.synchronize()
        word = int(st.item()) & 0xFFFFFFFF
    out, guards = arena.host()
    return word, guards, out, off


def record_verdicts(hs):
    """{golden key: status word} of every malformed container: run ONCE with the parent's library to write the golden file.  One word per codec, malformed kind
    and variant: every mixture, block size and block count must give the same."""
    words = {}
    for c in L.CODECS8:
        for m in L.MIXTURES:
            for B, n in L.SHAPES:
                for what in L.malformed_kinds(c):
                    for v in VARIANTS:
                        word = verdict(hs, L.malformed_container(c, m, B, n, what), v)[0]
                        assert words.setdefault(L.golden_key(c, what, v), word) == word, (c.key, m, B, n, what, v)
    return words


@pytest.mark.parametrize("codec, mixture", CASES, ids=lambda v: getattr(v, "key", v))
def test_malformed_blocks_end_as_the_parent_said(hs, codec, mixture):
    golden = json.load(open(GOLDEN))
    for B, blocks in L.SHAPES:
        for what in L.malformed_kinds(codec):
            fix = L.malformed_container(codec, mixture, B, blocks, what)
            for variant in VARIANTS:
                w = f"{codec.key} {mixture} B {B} x {blocks}, block {L.VICTIM} {what}, {variant} decode"
                word, guards, out, off = verdict(hs, fix, variant)
                assert word == golden[L.golden_key(codec, what, variant)], f"{w}: status {word:#x}"
                assert guards, f"{w}: bytes outside the output were written"
                if variant == "plain":      # (a lane per block: the neighbours of the refused block are decoded as ever)
                    lo, hi = L.VICTIM * B, (L.VICTIM + 1) * B
                    assert np.array_equal(out[:lo], fix.data[:lo]) and np.array_equal(out[hi:], fix.data[hi:]), f"{w}: a neighbour of the malformed block differs"
