"""Every decode variant on streams written from the packet grammar (tests/stream_grammar.py), not by an encoder: every field width that can hold its value,
the smallest legal counts, symbols sent again, pushes of listed symbols, references into lists with duplicates, every terminator form -- forms the reference
decoder accepts (tests/test_stream_grammar.py: the oracle's decoder and the compiled reference decode every stream used here) and no encoder of the kit writes.

Every case checks: status 0, the bytes equal to the INTENDED output (the writer's), 4 KiB guards on both sides of an output that starts 3 bytes behind a
16-byte boundary untouched, and the stream ring of the plain decode named through hs.decode_ring.  The helpers are those of test_gpu_decode_variants.py.

Packets that produce no byte (no literal, a zero-length run: the sym-aligned Packed codecs of 3 .. 16 byte symbols, the sym-aligned list codecs of wider
symbols) are the one legal form the GPU decoders REFUSE (include/hsrle.h): test_empty_packets_are_refused_by_every_variant pins that every
variant refuses them the same clean way."""
import numpy as np
import pytest

import decoder_fixtures as F
import stream_grammar as G
from hsrle_testlib import CODECS, CODEC_BY_KEY, GREEDY_CODECS
from test_gpu_decode_variants import PACKET_LIST, TAIL_CODECS, Arena, _check_blocks, _named_ring, _status, _upload, hs  # noqa: F401  (hs: the module's fixture)

pytestmark = pytest.mark.gpu

B = 4096
TUNINGS = ((0, 0, 0), (128, 64, 40), (256, 300, 16))
# one codec per header family: plain, Packed with the 7 bit range, sym-aligned Packed, list (LUT), Short, 128 bit
INDEX_CODECS = ("rle16_sym", "rle8_packed_multi", "rle24_sym_packed", "rle32_7symlut_sym", "rle24_3symlut_byte_short", "rle128_byte_packed")
MONO_CODECS = [c for c in CODECS if c not in GREEDY_CODECS]           # (a Greedy id decodes with the Short decoder of its grammar, which is in the list)
EMPTY_CODECS = [c for c in MONO_CODECS if G.grammar(c).has_empty]


def _window_ranges(fix):
    """Five ranges: from a position = 15 (mod 16) inside a W block, entirely inside the partial last block, from an odd offset of an X block into the block behind
    it, the first byte, the last byte."""
    U, nb = fix.U, len(fix.kinds)
    W = [b for b in F.blocks_of_kind(fix, "W") if b < nb - 1][0]
    X = [b for b in F.blocks_of_kind(fix, "X") if b + 1 < nb - 1][-1]
    last = (nb - 1) * B
    ranges = [(W * B + 16 * 37 + 15, 33), (last + 33, U - last - 33 - 9), (X * B + 1001, B - 1001 + 777), (0, 1), (U - 1, 1)]
    assert all(0 <= a and n > 0 and a + n <= U for a, n in ranges) and ranges[0][0] % 16 == 15 and ranges[1][0] + ranges[1][1] < U
    return ranges


def _split(hs, fix, container, info, arena, status, subs, what):
    import torch

    for sub in subs:
        ws = torch.full((max(hs.split_workspace_size(info, None, sub), 16),), 0xC3, dtype=torch.uint8, device="cuda")
        arena.reset()
        hs.decompress_split_async(container, info, arena.view, ws, status, sub_block=sub)
        _check_blocks(fix, arena, status, 0, info.blockCount, f"{what} split decode, sub-block {sub}")


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: c.key)
def test_grammar_containers(hs, codec):
    """The sparse (ring 64 for symbols of up to 4 bytes) and the dense (ring 128) container of three waves of 4 KiB blocks: the plain decode of the whole container
    and of the block ranges (63, 2), (1, 64), (last, 1); the split decode with a packet list, with entry records at every 512 bytes and with the library's
    choice; the windowed decode of five ranges."""
    import torch

    for layout in ("sparse", "dense"):
        fix = G.fixture(codec, layout)
        what = f"{codec.key} {layout}"
        ring = _named_ring(hs, fix, what)
        container, info = _upload(hs, fix)
        nb = info.blockCount
        assert nb == 3 * G.WAVE
        arena, status = Arena(fix.U), _status()
        for first, count in ((0, nb), (63, 2), (1, 64), (nb - 1, 1)):
            arena.reset()
            hs.decompress_async(container, info, arena.view, status, first_block=first, block_count=count)
            _check_blocks(fix, arena, status, first, count, f"{what} ring {ring} blocks [{first}, +{count})")
        _split(hs, fix, container, info, arena, status, (PACKET_LIST, 512, 0), what)
        runs = []
        for off, n in _window_ranges(fix):
            a, st = Arena(n), torch.zeros(4, dtype=torch.uint8, device="cuda")
            hs.decompress_range_dev_async(container, info, off, n, a.view, st)
            runs.append((off, n, a, st))
        torch.cuda.synchronize()
        for off, n, a, st in runs:
            w = f"{what} window [{off}, +{n}) = block {off // B} ({fix.kinds[off // B]}) + {off % B}"
            assert int.from_bytes(st.cpu().numpy().tobytes(), "little") == hs.MONO_DONE == 0, f"{w}: status"
            out, guards = a.host()
            assert np.array_equal(out, fix.data[off : off + n]), f"{w}: differs from the intended bytes"
            assert guards, f"{w}: bytes outside the output were written"


@pytest.mark.parametrize("key", TAIL_CODECS)
def test_block_size_384(hs, key):
    """The dense container of 384-byte blocks (no power of two: the row / tile arithmetic; the 128-byte ring): plain decode and the split decode of the library's choice."""
    codec = CODEC_BY_KEY[key]
    fix = G.fixture(codec, "dense", 384)
    assert _named_ring(hs, fix, key) == 128 and fix.ratio >= 0.40
    container, info = _upload(hs, fix)
    arena, status = Arena(fix.U), _status()
    hs.decompress_async(container, info, arena.view, status)
    _check_blocks(fix, arena, status, 0, info.blockCount, f"{key} B 384")
    _split(hs, fix, container, info, arena, status, (0,), f"{key} B 384")


@pytest.mark.parametrize("key", ("rle8_single", "rle8_packed_single"))
def test_single_ids_with_both_modes_interleaved(hs, key):
    """Even blocks in the multi-symbol grammar (mode byte 0), odd blocks in the Single grammar (mode byte 1) under the Single id: the mode is read per lane."""
    codec = CODEC_BY_KEY[key]
    for layout in ("sparse", "dense"):
        fix = G.fixture(codec, layout, modes=(0, 1))
        assert all(s[8] == i % 2 for i, s in enumerate(fix.streams) if fix.kinds[i] != "O"), "the 9th header byte is the mode"
        assert hs.decode_ring(key, fix.U, fix.payload_size) == (64 if layout == "sparse" else 128)
        container, info = _upload(hs, fix)
        arena, status = Arena(fix.U), _status()
        hs.decompress_async(container, info, arena.view, status)
        _check_blocks(fix, arena, status, 0, info.blockCount, f"{key} {layout}: modes 0 and 1 interleaved, plain decode")
        _split(hs, fix, container, info, arena, status, (PACKET_LIST, 512), f"{key} {layout}: modes 0 and 1 interleaved,")


def _dev_stream(stream):
    import torch

    t = torch.zeros(len(stream) + 64, dtype=torch.uint8, device="cuda")
    t[: len(stream)] = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    return t


def _mono_cases(codec):
    return [G.mono(codec)] + ([G.mono(codec, G.MONO_LONG, True)] if codec.key in G.MONO_LONG_CODECS else [])


@pytest.mark.parametrize("codec", MONO_CODECS, ids=lambda c: c.key)
def test_monolithic_streams(hs, codec):
    """ONE stream of the kinds W N X Z back to back (40 000 bytes; a few codecs also 300 000 with literal stretches of several KiB): the drop-in function of the
    reference's name under three tunings of the walk, the enqueue-only decode (DONE or NEEDS_REPAIR), then the synchronous device decode."""
    import torch

    for stream, want in _mono_cases(codec):
        U = len(want)
        what = f"{codec.key} monolithic {U}"
        try:
            for tuning in TUNINGS:
                hs.mono_tuning(*tuning)
                size, out = hs.call_dropin(codec.dname, stream, U)
                assert size == U and out == want, f"{what}: {codec.dname} under tuning {tuning} returns {size}" + ("" if size != U else ", wrong bytes")
        finally:
            hs.mono_tuning(0, 0, 0)
        t = _dev_stream(stream)
        arena = Arena(U)
        ws = torch.empty(max(hs.mono_decompress_workspace_size(codec.key, U, len(stream)), 256), dtype=torch.uint8, device="cuda")
        status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        n = hs.mono_decompress_dev_async(codec.key, t, stream[:16], arena.view, ws, status, stream_size=len(stream))
        torch.cuda.synchronize()
        out, guards = arena.host()
        assert n == U and guards, f"{what}: the enqueue-only decode wrote outside its output"
        assert int(status.item()) in (hs.MONO_DONE, hs.MONO_NEEDS_REPAIR), f"{what}: status {int(status.item())}"
        if int(status.item()) == hs.MONO_DONE:
            assert out.tobytes() == want, f"{what}: the enqueue-only decode says DONE, wrong bytes"
        arena.reset()
        got = hs.mono_decompress_dev(codec.key, t, dst=arena.view)
        out, guards = arena.host()
        assert got.numel() == U and out.tobytes() == want and guards, f"{what}: the synchronous device decode"


@pytest.mark.parametrize("key", INDEX_CODECS)
def test_monolithic_index_and_ranges(hs, key):
    """The persistent entry index at the library's spacing and at 512, and four range decodes from each."""
    import torch

    codec = CODEC_BY_KEY[key]
    stream, want = G.mono(codec)
    U, t = len(want), _dev_stream(stream)
    for spacing in (0, 512):
        index, info = hs.mono_index_build(key, t, spacing=spacing)
        assert info.uncompressedSize == U and info.compressedSize == len(stream)
        sp = info.spacing
        runs = []
        for off, n in ((0, U), (U - 1, 1), (3 * sp - 5, 10), (U // 2 + 7, 2 * sp + 77)):
            a, st = Arena(n), torch.full((4,), 0x4D, dtype=torch.uint8, device="cuda")
            hs.mono_decompress_range_dev_async(t, index, info, off, n, a.view, st)
            runs.append((off, n, a, st))
        torch.cuda.synchronize()
        for off, n, a, st in runs:
            what = f"{key} spacing {sp} range [{off}, +{n})"
            assert int.from_bytes(st.cpu().numpy().tobytes(), "little") == hs.MONO_DONE, f"{what}: status"
            out, guards = a.host()
            assert out.tobytes() == want[off : off + n] and guards, what


@pytest.mark.parametrize("codec", EMPTY_CODECS, ids=lambda c: c.key)
def test_empty_packets_are_refused_by_every_variant(hs, codec):
    """A packet without a literal whose run has zero bytes produces nothing; the reference walks over it, no encoder writes it, and every GPU decode variant
    refuses the stream that holds one (include/hsrle.h): a non-zero status word / MONO_MALFORMED / HSRLE_ERR_FORMAT / a drop-in result of 0, nothing written
    outside the output.  The blocks around it are ordinary grammar blocks."""
    import torch

    base = G.fixture(codec, "dense", blocks=5, last_len=B)
    stream, want = G.empty_packet_stream(codec)
    streams = list(base.streams)
    streams[2] = stream
    data = base.data.copy()
    data[2 * B : 3 * B] = np.frombuffer(want, dtype=np.uint8)
    fix = F.assemble(codec, "dense", B, data, base.kinds, streams)
    container, info = _upload(hs, fix)
    arena, status = Arena(fix.U), _status()

    def refused(what):
        torch.cuda.synchronize()
        assert int(status.item()) != 0, f"{codec.key}: {what} accepts a stream with empty packets"
        assert arena.host()[1], f"{codec.key}: {what} wrote outside the output"
        status.zero_()
        arena.reset()

    hs.decompress_async(container, info, arena.view, status)
    refused("the block decode")
    for sub in (PACKET_LIST, 512):
        ws = torch.full((max(hs.split_workspace_size(info, None, sub), 16),), 0xC3, dtype=torch.uint8, device="cuda")
        hs.decompress_split_async(container, info, arena.view, ws, status, sub_block=sub)
        refused(f"the split decode, sub-block {sub}")
    a, st = Arena(B), torch.zeros(4, dtype=torch.uint8, device="cuda")
    hs.decompress_range_dev_async(container, info, 2 * B, B, a.view, st)
    torch.cuda.synchronize()
    assert int.from_bytes(st.cpu().numpy().tobytes(), "little") != 0 and a.host()[1], f"{codec.key}: the windowed decode"
    # the same stream as ONE monolithic stream
    assert hs.call_dropin(codec.dname, stream, B)[0] == 0, f"{codec.key}: {codec.dname} accepts a stream with empty packets"
    t = _dev_stream(stream)
    ws = torch.empty(max(hs.mono_decompress_workspace_size(codec.key, B, len(stream)), 256), dtype=torch.uint8, device="cuda")
    mstatus = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    a = Arena(B)
    hs.mono_decompress_dev_async(codec.key, t, stream[:16], a.view, ws, mstatus, stream_size=len(stream))
    torch.cuda.synchronize()
    assert int(mstatus.item()) == hs.MONO_MALFORMED and a.host()[1], f"{codec.key}: the enqueue-only monolithic decode says {int(mstatus.item())}"
    with pytest.raises(hs.HsrleError):
        hs.mono_decompress_dev(codec.key, t, dst=a.view)
    assert a.host()[1], f"{codec.key}: the synchronous monolithic decode wrote outside the output"
