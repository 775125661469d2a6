"""Every decode variant on host-built mixed containers (tests/decoder_fixtures.py): block streams from the CPU oracle, assembled by
hsrle_testlib.build_container, independent of the GPU encoders -- the ratio, and with it the stream ring of the plain decode, and the make-up of every
wave of 64 lanes are fixed by construction: a few literal-only and packet-dense blocks beside neighbours that finish after one packet.

Which kernel a test runs is said by hs.decode_ring (plain decode: the 64- or the 128-byte ring instantiation of k_decode_blocks) or by the variant itself
(windowed decode, decode from entry records, packet list: always the 128-byte ring); every test asserts it.

Every decode here writes into an output that starts 3 bytes behind a 16-byte boundary inside a larger buffer filled with 0xA5, with at least 4096 bytes
of guard on both sides that must stay 0xA5; the status word starts as 0 and must end as 0; the bytes are compared with the HOST input."""
import numpy as np
import pytest

import decoder_fixtures as F
from hsrle_testlib import CODECS, CODEC_BY_KEY

pytestmark = pytest.mark.gpu

PACKET_LIST = 1          # include/hsrle.h: HSRLE_SPLIT_PACKET_LIST
GUARD, SHIFT, FILL = 4096, 3, 0xA5

TAIL_CODECS = ("rle8_packed_multi", "rle8_7symlut", "rle8_packed_single", "rle8_3symlut_short", "rle8_single_short", "rle16_sym", "rle24_3symlut_byte", "rle32_byte_packed",
               "rle48_7symlut_byte_short", "rle64_3symlut_byte", "rle64_7symlut_byte_short_greedy", "rle128_sym_packed")
TAIL_LENGTHS = lambda B: (1, 15, 16, 17, 127, 129, B - 1)
SAME_AS_LIBRARY = ("rle8_packed_multi", "rle8_7symlut", "rle16_sym", "rle32_byte_packed", "rle64_3symlut_byte", "rle128_sym_packed")


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    return hsrle


class Arena:
    """An output of n bytes at byte offset 3 (mod 16) inside a larger buffer of 0xA5, GUARD bytes and more on both sides."""

    def __init__(self, n):
        import torch

        self.lo = GUARD + SHIFT
        self.buf = torch.full((self.lo + n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.resize(n)
        assert self.view.data_ptr() % 16 == SHIFT

    def resize(self, n):
        """An output of fewer bytes in the same buffer: what follows it is guard."""
        assert self.lo + n + GUARD <= self.buf.numel()
        self.n, self.view = n, self.buf[self.lo : self.lo + n]

    def reset(self):
        self.buf.fill_(FILL)

    def host(self):
        """(the output bytes, True if both guards still hold 0xA5) -- after a synchronise"""
        h = self.buf.cpu().numpy()
        return h[self.lo : self.lo + self.n], bool((h[: self.lo] == FILL).all() and (h[self.lo + self.n :] == FILL).all())


def _upload(hs, fix):
    """The host-built container in device memory and its info (read and validated from the host bytes by the library)."""
    import torch

    return torch.frombuffer(bytearray(fix.container), dtype=torch.uint8).cuda(), hs.container_info(fix.container)


def _status():
    import torch

    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _check_blocks(fix, arena, status, first, count, what):
    """Blocks [first, first + count) hold the host input, every other byte of the output and the guards 0xA5, the status word 0."""
    import torch

    torch.cuda.synchronize()
    assert int(status.item()) == 0, f"{what}: status {int(status.item()):#x}"
    out, guards = arena.host()
    lo, hi = first * fix.B, min((first + count) * fix.B, fix.U)
    if not np.array_equal(out[lo:hi], fix.data[lo:hi]):
        bad = lo + int(np.flatnonzero(out[lo:hi] != fix.data[lo:hi])[0])
        raise AssertionError(f"{what}: first wrong byte at {bad} = block {bad // fix.B} ({fix.kinds[bad // fix.B]}) + {bad % fix.B}")
    assert bool((out[:lo] == FILL).all() and (out[hi:] == FILL).all()), f"{what}: a block outside the range was written"
    assert guards, f"{what}: bytes outside the output were written"


def _named_ring(hs, fix, what):
    ring = hs.decode_ring(fix.codec.key, fix.U, fix.payload_size)
    assert ring == F.expected_ring(fix), f"{what}: the plain decode of this container takes the {ring}-byte ring, the fixture was built for {F.expected_ring(fix)}"
    return ring


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# 1. plain decode: both rings for every codec of 1 .. 4 byte symbols


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: c.key)
def test_plain_decode_both_rings_and_block_ranges(hs, codec):
    """hsrle_decompress_blocks_dev_async on the sparse (ring 64 for S <= 4) and the dense (ring 128) containers of 4 KiB and 16 KiB blocks; on the 4 KiB
    ones also block ranges: two lanes from a first block that is no multiple of 64 (blocks 63 and 64), 64 blocks from block 1, the partial last block alone, five whole blocks
    from a literal-only block on."""
    rings = set()
    for B in (4096, 16384):
        for layout in ("sparse", "dense"):
            fix = F.fixture(codec, layout, B)
            what = f"{codec.key} {layout} B {B}"
            ring = _named_ring(hs, fix, what)
            rings.add(ring)
            container, info = _upload(hs, fix)
            nb = info.blockCount
            ranges = [(0, nb)]
            if B == 4096:
                from_literal = [b for b in F.blocks_of_kind(fix, "L") if b + 5 <= nb - 1][1]
                ranges += [(63, 2), (1, 64), (nb - 1, 1), (from_literal, 5)]
            arena, status = Arena(fix.U), _status()
            for first, count in ranges:
                arena.reset()
                hs.decompress_async(container, info, arena.view, status, first_block=first, block_count=count)
                _check_blocks(fix, arena, status, first, count, f"{what} ring {ring} blocks [{first}, +{count})")
    assert rings == ({64, 128} if codec.S <= 4 else {128})


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# 2. tail matrix


@pytest.mark.parametrize("key", TAIL_CODECS)
def test_tail_matrix(hs, key):
    """Containers of exactly 64 blocks (one full workgroup) and of 65 (the second workgroup has ONE active lane); the last block 1, 15, 16, 17, 127, 129 or
    B - 1 bytes of literals, of one symbol or of back-to-back short runs.  B = 4096: sparse and dense; B = 384: the row / tile arithmetic for a block size
    that is no power of two (dense only -- sparse containers are not built below 2048 -- and the 128-byte ring)."""
    codec = CODEC_BY_KEY[key]
    status = _status()
    for B in (4096, 384):
        for layout in (("sparse", "dense") if B == 4096 else ("dense",)):
            for blocks in (64, 65):
                arena = Arena((blocks - 1) * B + B - 1)
                for fix in F.tail_matrix(codec, layout, B, blocks, TAIL_LENGTHS(B)):
                    what = f"{key} {layout} B {B}: {blocks} blocks, the last {fix.U - (blocks - 1) * B} bytes of {fix.kinds[-1]}"
                    ring = _named_ring(hs, fix, what)
                    assert B != 384 or ring == 128
                    container, info = _upload(hs, fix)
                    assert info.blockCount == blocks
                    arena.reset()
                    arena.resize(fix.U)
                    hs.decompress_async(container, info, arena.view, status)
                    _check_blocks(fix, arena, status, 0, blocks, f"{what} ring {ring}")


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# 3. windowed decode (WIN = true instantiations; always the 128-byte ring)


def _window_ranges(fix):
    B, U, nb = fix.B, fix.U, len(fix.kinds)
    lits = [b for b in F.blocks_of_kind(fix, "L") if b + 1 < nb - 1]
    dense = [b for b in F.blocks_of_kind(fix, "D") if b < nb - 1]
    L, D = lits[len(lits) // 2], dense[len(dense) // 2]
    last = (nb - 1) * B
    ranges = [(0, U), (0, 1), (U - 1, 1),
              (L * B + 1001, B - 1001 + 777),              # from an odd offset inside a literal-only block into the block behind it
              (last + 33, U - last - 33 - 9),              # entirely inside the partial last block
              (D * B, B)]                                  # exactly one block
    ranges += [(D * B + 16 * 37 + 15, n) for n in (2, 17, 33)]   # from a position = 15 (mod 16) inside a packet-dense block
    assert all(0 <= a and n > 0 and a + n <= U for a, n in ranges) and (L * B + 1001) % 2 == 1
    return ranges


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: c.key)
def test_windowed_decode(hs, codec):
    """hsrle_decompress_range_dev_async on the sparse 4 KiB container; every range is enqueued before the one synchronise."""
    import torch

    fix = F.fixture(codec, "sparse", 4096)
    _named_ring(hs, fix, codec.key)            # (of the container's PLAIN decode; the windowed launch takes the 128-byte ring whatever the ratio)
    container, info = _upload(hs, fix)
    runs = []
    for off, n in _window_ranges(fix):
        arena, status = Arena(n), torch.zeros(4, dtype=torch.uint8, device="cuda")
        hs.decompress_range_dev_async(container, info, off, n, arena.view, status)
        runs.append((off, n, arena, status))
    torch.cuda.synchronize()
    for off, n, arena, status in runs:
        what = f"{codec.key} window [{off}, +{n}) = block {off // fix.B} ({fix.kinds[off // fix.B]}) + {off % fix.B}"
        assert int.from_bytes(status.cpu().numpy().tobytes(), "little") == hs.MONO_DONE == 0, f"{what}: status"
        out, guards = arena.host()
        assert np.array_equal(out, fix.data[off : off + n]), f"{what}: differs from the input"
        assert guards, f"{what}: bytes outside the output were written"


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# 4. split decode: packet list, entry records at every 512 bytes, the library's choice


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: c.key)
def test_split_decode(hs, oracle, codec):
    """hsrle_decompress_split_dev_async on the sparse and the dense 4 KiB containers.  Packet list (also the library's choice, 0, for such a container): for
    S = 1 every D block has more run packets than its list holds (B / 8 + 2 entries; counted here by the oracle's decoder), so the walking lane's
    close-and-finish path runs beside Z blocks of one packet.  512: k_decode_blocks from entry records, eight lanes per block (the 128-byte ring)."""
    import ctypes
    import torch

    for layout in ("sparse", "dense"):
        fix = F.fixture(codec, layout, 4096)
        _named_ring(hs, fix, f"{codec.key} {layout}")
        container, info = _upload(hs, fix)
        assert hs.lib().hsrle_split_sub_block_size(ctypes.byref(info), 0) == PACKET_LIST
        if codec.S == 1:
            dense = [b for b in F.blocks_of_kind(fix, "D") if b + 1 < len(fix.kinds)]
            assert dense and all(oracle.run_packets(codec, fix.streams[b], 4096) > 4096 // 8 + 2 for b in dense), f"{codec.key} {layout}: a D block fits its packet list"
        arena, status = Arena(fix.U), _status()
        for sub in (PACKET_LIST, 512, 0):
            ws = torch.full((max(hs.split_workspace_size(info, None, sub), 16),), 0xC3, dtype=torch.uint8, device="cuda")
            arena.reset()
            hs.decompress_split_async(container, info, arena.view, ws, status, sub_block=sub)
            _check_blocks(fix, arena, status, 0, info.blockCount, f"{codec.key} {layout} split decode, sub-block {sub}")


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# 5. both modes of the 8 bit plain / Packed grammar under one Single id


@pytest.mark.parametrize("single, multi", (("rle8_single", "rle8_multi"), ("rle8_packed_single", "rle8_packed_multi")))
def test_mixed_modes_under_a_single_id(hs, oracle, single, multi):
    """A container with the Single codec's id whose even blocks are the multi-symbol encoder's streams (mode byte 0) and whose odd blocks are the Single
    encoder's (mode byte 1).  include/hsrle.h does not forbid it: a block is "a complete reference stream", and the reference's rle8_decompress /
    rle8_packed_decompress read the mode from the stream -- so k_decode_blocks (SGL), the packet walk and the record walk must read it per lane."""
    import torch

    cs, cm = CODEC_BY_KEY[single], CODEC_BY_KEY[multi]
    for layout in ("sparse", "dense"):
        base = F.fixture(cs, layout, 4096)
        a, b = oracle.compress_blocks(cm, base.data, 4096), base.streams
        streams = [a[i] if i % 2 == 0 else b[i] for i in range(len(b))]
        assert all(s[8] == i % 2 for i, s in enumerate(streams)), "the 9th header byte is the mode"
        fix = F.assemble(cs, layout, 4096, base.data, base.kinds, streams)
        assert hs.decode_ring(single, fix.U, fix.payload_size) == (64 if layout == "sparse" else 128)
        container, info = _upload(hs, fix)
        arena, status = Arena(fix.U), _status()
        hs.decompress_async(container, info, arena.view, status)
        _check_blocks(fix, arena, status, 0, info.blockCount, f"{single} {layout}: modes 0 and 1 interleaved, plain decode")
        for sub in (PACKET_LIST, 512):
            ws = torch.full((max(hs.split_workspace_size(info, None, sub), 16),), 0xC3, dtype=torch.uint8, device="cuda")
            arena.reset()
            hs.decompress_split_async(container, info, arena.view, ws, status, sub_block=sub)
            _check_blocks(fix, arena, status, 0, info.blockCount, f"{single} {layout}: modes 0 and 1 interleaved, split decode {sub}")


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# 6. the host-built container is the library's


@pytest.mark.parametrize("key", SAME_AS_LIBRARY)
def test_host_built_container_is_the_librarys(hs, key):
    """build_container's claim ("exactly as the device does"), and with it every test above: hs.compress of the dense 4 KiB input returns the very bytes."""
    import torch

    fix = F.fixture(CODEC_BY_KEY[key], "dense", 4096)
    src = torch.from_numpy(fix.data.copy()).cuda()
    container, info = hs.compress(key, src, block_size=4096)
    assert container.cpu().numpy().tobytes() == fix.container, f"{key}: the library's container differs from the host-built one"
    ring = _named_ring(hs, fix, key)
    arena, status = Arena(fix.U), _status()
    hs.decompress_async(container, info, arena.view, status)
    _check_blocks(fix, arena, status, 0, info.blockCount, f"{key} ring {ring}: the library's own container")
