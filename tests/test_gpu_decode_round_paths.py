"""The two ends of a decode round of k_decode_blocks: the full-row flush (one wave-uniform test: all 64 lanes active, each with exactly T bytes behind one
common base; then no exchange, no per-store predicate) beside the general flush it leaves for partial waves, block tails and lanes that ended in an error, and
the top-up's one predicate region per chunk register.

KB-sized host-built containers (tests/decoder_fixtures.py: block streams from the CPU oracle, so the expected bytes are the fixture's input); every decode
writes into an output with 256 guard bytes of 0xA5 on both sides that must stay 0xA5.  The uncapped decoders (8 bit without the Short families, 128 bit) have
the full-row path; rle32_byte (capped rounds: 64-byte halves, never that path) is the control."""
import struct

import numpy as np
import pytest

import decoder_fixtures as F
import stream_grammar as G
from hsrle_testlib import CODEC_BY_KEY

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
DEC_ERR_HEADER, DEC_ERR_STREAM = 1, 2      # csrc/hsrle_decode.hip.h: DecodeError
UNCAPPED = ("rle8_packed_multi", "rle8_multi", "rle8_3symlut", "rle128_sym")
KEYS = UNCAPPED + ("rle32_byte",)
B = 384                                    # three rounds of 128 bytes per block
TAILS = (1, 15, 16, 17, 127, 128, 129, 383)


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    return hsrle


class Guarded:
    """An output of n bytes with GUARD bytes of 0xA5 on both sides."""

    def __init__(self, n):
        import torch

        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.view = self.buf[GUARD : GUARD + n]

    def host(self):
        """(the output bytes, True if both guards still hold 0xA5) -- after a synchronise"""
        h = self.buf.cpu().numpy()
        return h[GUARD : GUARD + self.n], bool((h[:GUARD] == FILL).all() and (h[GUARD + self.n :] == FILL).all())


def _upload(hs, fix):
    import torch

    return torch.frombuffer(bytearray(fix.container), dtype=torch.uint8).cuda(), hs.container_info(fix.container)


def _plain_decode(hs, fix):
    """(output bytes, guards intact, status word) of hsrle_decompress_blocks_dev_async on the whole container"""
    import torch

    container, info = _upload(hs, fix)
    out, status = Guarded(fix.U), torch.zeros(1, dtype=torch.int32, device="cuda")
    hs.decompress_async(container, info, out.view, status)
    torch.cuda.synchronize()
    got, guards = out.host()
    return got, guards, int(status.item())


def _assert_exact(hs, fix, what):
    got, guards, status = _plain_decode(hs, fix)
    assert status == 0, f"{what}: status {status:#x}"
    if not np.array_equal(got, fix.data):
        bad = int(np.flatnonzero(got != fix.data)[0])
        raise AssertionError(f"{what}: first wrong byte at {bad} = block {bad // fix.B} ({fix.kinds[bad // fix.B]}) + {bad % fix.B}")
    assert guards, f"{what}: bytes outside the output were written"


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. path selection


@pytest.mark.parametrize("key", KEYS)
def test_path_selection(hs, key):
    """Dense containers of 384-byte blocks.  64 blocks: every round of the one workgroup is a full-row round.  65: the second workgroup has one active lane
    and never takes the path.  128 blocks, the last of 1 .. 383 bytes: the last workgroup leaves the path in its final rounds (a last block of 128 or 129 bytes:
    after one full-row round), and the tail bytes are written."""
    codec = CODEC_BY_KEY[key]
    for blocks in (64, 65):
        fix = F.fixture(codec, "dense", B, blocks=blocks, last_len=B)
        assert fix.U == blocks * B and hs.decode_ring(key, fix.U, fix.payload_size) == 128
        _assert_exact(hs, fix, f"{key}: {blocks} whole blocks")
    for fix in F.tail_matrix(codec, "dense", B, 128, TAILS, last_kinds="LD"):
        _assert_exact(hs, fix, f"{key}: 128 blocks, the last {fix.U - 127 * B} bytes of {fix.kinds[-1]}")


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. both rings


@pytest.mark.parametrize("key", KEYS)
def test_both_rings(hs, key):
    """Sparse containers of 2048-byte blocks take the 64-byte stream ring (symbols of up to 4 bytes): 64 whole blocks, and 64 with a last block of 2047 bytes."""
    codec = CODEC_BY_KEY[key]
    for last in (2048, 2047):
        fix = F.fixture(codec, "sparse", 2048, blocks=64, last_len=last)
        ring = hs.decode_ring(key, fix.U, fix.payload_size)
        assert ring == F.expected_ring(fix) == (64 if codec.S <= 4 else 128)
        _assert_exact(hs, fix, f"{key}: sparse, 64 blocks of 2048, the last {last}, ring {ring}")


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. an error lane among full rows


def _packets(g, stream):
    """[(header offset, output position)] of every packet of a plain / Packed (7 bit range) / list stream, the terminator included"""
    s, p, o, res = bytes(stream), g.header, 0, []

    def ext(n):
        nonlocal p
        p += n
        return int.from_bytes(s[p - n : p], "little")

    while True:
        res.append((p, o))
        if g.kind == "lut":
            v = ext(2)
            idx, cf, rf = v >> (14 if g.K == 3 else 13), (v >> g.RB) & 0x7F, v & ((1 << g.RB) - 1)
            p += g.S if idx == g.K else 0
            cnt = cf if cf >= 2 else ext(2 if cf == 1 else 4)
            rng = rf if rf >= 2 else ext(2 if rf == 1 else 4)
            end = rf == 1 and rng == 0
        elif g.kind == "packed":
            assert g.range7
            b = ext(1)
            cnt = (b & 0x7F) or ext(4)
            p += 0 if b & 0x80 else g.S
            rng = ext(4 if s[p] & 1 else 1)
            end, rng = rng == 1, rng >> 1
        else:
            assert g.kind == "plain"
            p += g.S
            cnt = ext(1) or ext(4)
            r0 = ext(1)
            rng = r0 or ext(4)
            end = r0 == 0 and rng == 0
        lit = 0 if end else max(rng - g.bias, 0)
        p, o = p + lit, o + lit
        if end or cnt == 0:
            return res
        o += g.run_bytes(cnt)


def _long_range_header(g):
    """A packet header in the long-range form whose literal count no stream of these containers holds"""
    w, huge = G.Writer(g), 0x3FFFFFF0
    if g.kind == "lut":
        return w._word(g.K, 2, huge, "d", "u32", False, bytes(g.S))
    return w._plain_fields(2, "d", huge, "u32", 0, bytes(g.S))


@pytest.mark.parametrize("variant", ("stream size field", "long range"))
@pytest.mark.parametrize("key", KEYS)
def test_error_lane_among_full_rows(hs, key, variant):
    """One bad block among 64 of 384 bytes.  Its stream-size header field off by one: DEC_ERR_HEADER, the lane never has a full row, so no round of the
    workgroup is a full-row round.  A packet header about a third into the block rewritten to a long-range form whose literal count exceeds the stream:
    DEC_ERR_STREAM after full-row rounds -- what the block decoded before it is flushed (checked: its first 128 bytes).  The status carries the bit, the other
    63 blocks are exact, the guards untouched."""
    codec = CODEC_BY_KEY[key]
    g = G.grammar(codec)
    good = F.fixture(codec, "dense", B, blocks=64, last_len=B)
    bad = F.blocks_of_kind(good, "D")[1]
    stream = bytearray(good.streams[bad])
    if variant == "stream size field":
        struct.pack_into("<I", stream, 4, len(stream) + 1)
        bit, intact = DEC_ERR_HEADER, 0
    else:
        at, pos = next((a, o) for a, o in _packets(g, stream) if o >= B // 3 + 16)
        hdr = _long_range_header(g)
        assert B // 3 < pos < B - 16 and at + len(hdr) <= len(stream), "the packet to rewrite lies inside the block's second round"
        stream[at : at + len(hdr)] = hdr
        bit, intact = DEC_ERR_STREAM, 128
    streams = list(good.streams)
    streams[bad] = bytes(stream)
    fix = F.assemble(codec, "dense", B, good.data, good.kinds, streams)
    got, guards, status = _plain_decode(hs, fix)
    what = f"{key}, block {bad} with a bad {variant}"
    assert status & bit, f"{what}: status {status:#x}"
    lo, hi = bad * B, (bad + 1) * B
    assert np.array_equal(got[:lo], good.data[:lo]) and np.array_equal(got[hi:], good.data[hi:]), f"{what}: another block's bytes differ from the input"
    assert np.array_equal(got[lo : lo + intact], good.data[lo : lo + intact]), f"{what}: the rows the block completed before the error"
    assert guards, f"{what}: bytes outside the output were written"


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. neighbour variants that share the flush


@pytest.mark.parametrize("key", KEYS)
def test_range_and_split_decode(hs, key):
    """On the container of 64 blocks of 384 bytes: the range decode of [B + 5, 63 B - 7) (the instantiation with an output window: general flush only), and the
    split decode with sub-blocks of 128 bytes (lanes from entry records, three per block, one round each)."""
    import torch

    codec = CODEC_BY_KEY[key]
    fix = F.fixture(codec, "dense", B, blocks=64, last_len=B)
    container, info = _upload(hs, fix)
    off, n = B + 5, 62 * B - 12
    out, st = Guarded(n), torch.zeros(4, dtype=torch.uint8, device="cuda")
    hs.decompress_range_dev_async(container, info, off, n, out.view, st)
    torch.cuda.synchronize()
    got, guards = out.host()
    assert int.from_bytes(st.cpu().numpy().tobytes(), "little") == hs.MONO_DONE == 0, f"{key}: range decode status"
    assert np.array_equal(got, fix.data[off : off + n]), f"{key}: range decode [{off}, +{n}) differs from the input"
    assert guards, f"{key}: range decode wrote outside the output"

    out, status = Guarded(fix.U), torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.full((max(hs.split_workspace_size(info, None, 128), 16),), 0xC3, dtype=torch.uint8, device="cuda")
    hs.decompress_split_async(container, info, out.view, ws, status, sub_block=128)
    torch.cuda.synchronize()
    got, guards = out.host()
    assert int(status.item()) == 0, f"{key}: split decode status {int(status.item()):#x}"
    assert np.array_equal(got, fix.data), f"{key}: split decode, sub-block 128, differs from the input"
    assert guards, f"{key}: split decode wrote outside the output"
