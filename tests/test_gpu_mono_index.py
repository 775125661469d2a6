"""Seekable monolithic streams (include/hsrle.h): a persistent entry-point index beside ONE monolithic reference stream
(hsrle_mono_index_build_dev), byte-range decode from it (hsrle_mono_decompress_range_dev_async), and byte-range decode of block containers
(hsrle_decompress_range_dev_async).  Bar: every range equals the slice of what the oracle's (= the reference's) encoder was given, dOut may
sit at any byte address, and nothing outside dOut[0, length) is ever written; the index is position independent, deterministic and can be
stored and loaded again; a stale or foreign index says INDEX_MISMATCH, a corrupted stream MALFORMED; the range decode is graph-capturable."""
import random

import numpy as np
import pytest

from hsrle_testlib import CODECS, CODEC_BY_KEY, SYNTH_RUNS, SYNTH_VIDEO, mixed_runs

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    yield hsrle
    hsrle.mono_tuning(0, 0, 0)


def _dev_stream(stream, at=0):
    """The stream at byte `at` (a multiple of 128) of a fresh allocation, 64 zero bytes of slack behind it."""
    import torch

    t = torch.zeros(at + len(stream) + 64, dtype=torch.uint8, device="cuda")
    t[at : at + len(stream)] = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
    return t[at:]


def _mixed(oracle, S, seed, size):
    """Run-distributed data, then video-shaped data: both packet mixes in one stream."""
    half = size // 2
    return np.concatenate([oracle.synth(SYNTH_RUNS, S, seed, half), oracle.synth(SYNTH_VIDEO, S, seed + 1, size - half)])


class _Out:
    """dOut at an odd byte address inside a buffer of 0xA5 bytes: GUARD bytes in front, GUARD behind."""

    def __init__(self, length):
        import torch

        self.length = length
        self.buf = torch.full((length + 2 * GUARD + 1,), 0xA5, dtype=torch.uint8, device="cuda")
        self.view = self.buf[GUARD + 1 : GUARD + 1 + length]
        assert self.view.data_ptr() % 2 == 1

    def guards_hold(self):
        return bool((self.buf[: GUARD + 1] == 0xA5).all()) and bool((self.buf[GUARD + 1 + self.length :] == 0xA5).all())

    def untouched(self):
        return bool((self.buf == 0xA5).all())


def _status():
    import torch

    return torch.full((4,), 0x4D, dtype=torch.uint8, device="cuda")


def _word(status):
    return int.from_bytes(status.cpu().numpy().tobytes()[:4], "little")


def _ranges(usize, spacing, seed, count=12):
    rng = random.Random(seed)
    r = [(0, usize), (0, 1), (usize - 1, 1), (rng.randrange(usize), 1), (0, min(usize, 1000)), (max(0, usize - 3000), min(usize, 3000))]
    for k in (1, 2, usize // spacing // 2):                                 # across a spacing boundary
        b = k * spacing
        if 5 <= b < usize - 5:
            r.append((b - 5, 10))
            r.append((b - 1, 2))
    for _ in range(count):
        a = rng.randrange(usize)
        r.append((a, rng.randrange(1, min(usize - a, 3 * spacing + 77) + 1)))
    return r


def _check_ranges(hs, stream_t, index, info, src, ranges):
    """Enqueue every range, then compare each with the slice of the input and check its guards."""
    import torch

    outs = []
    for off, n in ranges:
        o, st = _Out(n), _status()
        hs.mono_decompress_range_dev_async(stream_t, index, info, off, n, o.view, st)
        outs.append((off, n, o, st))
    torch.cuda.synchronize()
    for off, n, o, st in outs:
        assert _word(st) == hs.MONO_DONE, f"range [{off}, +{n}): status {_word(st)}"
        assert torch.equal(o.view, src[off : off + n]), f"range [{off}, +{n}) differs"
        assert o.guards_hold(), f"range [{off}, +{n}): bytes outside dOut were written"


@pytest.mark.parametrize("key", [c.key for c in CODECS])
def test_range_decode_every_codec(hs, oracle, key):
    import torch

    codec = CODEC_BY_KEY[key]
    data = _mixed(oracle, codec.S, 5, (2 << 20) + 777)
    stream = oracle.compress(codec, data.tobytes())
    t = _dev_stream(stream)
    index, info = hs.mono_index_build(key, t, spacing=256)
    assert info.uncompressedSize == data.size and info.compressedSize == len(stream) and info.spacing == 256
    assert info.recordCount == (data.size + 255) // 256 and index.numel() == 64 + 96 * info.recordCount
    src = torch.from_numpy(data).cuda()
    _check_ranges(hs, t, index, info, src, _ranges(data.size, 256, seed=hash(key) & 0xFFFF))


def test_index_spacing_and_library_choice(hs, oracle):
    """spacing 0 = the library's choice; larger spacings give the same bytes."""
    import torch

    codec = CODEC_BY_KEY["rle16_3symlut_byte"]
    data = _mixed(oracle, codec.S, 8, (3 << 20) + 5)
    stream = oracle.compress(codec, data.tobytes())
    t = _dev_stream(stream)
    src = torch.from_numpy(data).cuda()
    for spacing in (0, 128, 4096, 1 << 20):
        index, info = hs.mono_index_build(codec.key, t, spacing=spacing)
        assert info.spacing % 128 == 0 and (spacing == 0 or info.spacing == spacing)
        assert index.numel() == hs.mono_index_size(codec.key, data.size, len(stream), spacing)
        _check_ranges(hs, t, index, info, src, _ranges(data.size, info.spacing, seed=spacing, count=4))


def test_index_is_position_independent_and_persistent(hs, oracle):
    import torch

    key = "rle32_7symlut_byte"
    codec = CODEC_BY_KEY[key]
    data = _mixed(oracle, codec.S, 11, (3 << 20) + 99)
    stream = oracle.compress(codec, data.tobytes())
    t = _dev_stream(stream)
    index, info = hs.mono_index_build(key, t, spacing=512)
    blob = index.cpu().numpy().tobytes()                                  # the sidecar file

    loaded = hs.mono_index_info(blob)
    assert (loaded.codec, loaded.uncompressedSize, loaded.compressedSize, loaded.spacing, loaded.recordCount, loaded.indexBytes) == \
           (info.codec, info.uncompressedSize, info.compressedSize, info.spacing, info.recordCount, info.indexBytes)
    assert bytes(loaded.streamHead) == stream[:16]
    with pytest.raises(hs.HsrleError):
        hs.mono_index_info(blob[:-1])                                     # truncated
    with pytest.raises(hs.HsrleError):
        hs.mono_index_info(b"X" + blob[1:])                               # flipped magic
    with pytest.raises(hs.HsrleError):
        hs.mono_index_info(blob[:32])

    idx2 = torch.empty(len(blob) + 16, dtype=torch.uint8, device="cuda")[16:]   # another buffer, another address
    idx2.copy_(torch.frombuffer(bytearray(blob), dtype=torch.uint8))
    t2 = _dev_stream(stream, at=384)                                      # the stream at another 128-aligned address
    src = torch.from_numpy(data).cuda()
    ranges = _ranges(data.size, 512, seed=3)
    _check_ranges(hs, t, index, info, src, ranges)
    _check_ranges(hs, t2, idx2, loaded, src, ranges)
    # built again at the other address: the same bytes
    again, _ = hs.mono_index_build(key, t2, spacing=512)
    assert again.cpu().numpy().tobytes() == blob


@pytest.mark.parametrize("key", ["rle8_multi", "rle24_3symlut_sym", "rle16_sym_short", "rle64_byte"])
def test_index_is_deterministic_under_repairs(hs, oracle, key):
    """Random literals between runs (tests/test_gpu_mono_async.py: the first try needs repair there): the index bytes do not depend on the
    region size or look-back of the walk, nor on the number of repair rounds."""
    import torch

    codec = CODEC_BY_KEY[key]
    rng = random.Random(99)
    parts = []
    while sum(map(len, parts)) < (2 << 20):
        parts.append(bytes(rng.randrange(256) for _ in range(rng.choice([1, 7, 130, 300, 700]))))
        parts.append(mixed_runs(rng, rng.choice([40, 200, 1000])))
    data = np.frombuffer(b"".join(parts)[: 2 << 20], dtype=np.uint8)
    stream = oracle.compress(codec, data.tobytes())
    t = _dev_stream(stream)
    blobs = []
    try:
        for region, lookback in ((64, 16), (0, 0), (8192, 4096)):
            hs.mono_tuning(0, region, lookback)
            index, info = hs.mono_index_build(key, t, spacing=512)
            blobs.append(index.cpu().numpy().tobytes())
    finally:
        hs.mono_tuning(0, 0, 0)
    assert blobs[0] == blobs[1] == blobs[2]
    src = torch.from_numpy(data).cuda()
    _check_ranges(hs, t, index, info, src, _ranges(data.size, 512, seed=7, count=6))


def _enqueue_one(hs, t, index, info, off, n):
    import torch

    o, st = _Out(n), _status()
    hs.mono_decompress_range_dev_async(t, index, info, off, n, o.view, st)
    torch.cuda.synchronize()
    return o, _word(st)


def test_index_mismatch_and_malformed(hs, oracle):
    import torch

    key = "rle8_packed_multi"
    codec = CODEC_BY_KEY[key]
    a = oracle.synth(SYNTH_RUNS, 1, 21, 4 << 20)
    sa = oracle.compress(codec, a.tobytes())
    ta = _dev_stream(sa)
    index, info = hs.mono_index_build(key, ta, spacing=4096)

    # another stream, another header: nothing is written
    other = oracle.compress(codec, oracle.synth(SYNTH_RUNS, 1, 22, 4 << 20).tobytes())
    assert other[:16] != sa[:16]
    o, st = _enqueue_one(hs, _dev_stream(other), index, info, 12345, 100000)
    assert st == hs.MONO_INDEX_MISMATCH and o.untouched()

    # the same header, other content behind it: the same runs with other symbols in the second half (the packets keep their lengths)
    b = a.copy()
    b[a.size // 2 :] ^= np.uint8(0x5A)
    sb = oracle.compress(codec, b.tobytes())
    if len(sb) != len(sa):
        pytest.skip("streams of different sizes")
    assert sb[:16] == sa[:16] and sb != sa
    o, st = _enqueue_one(hs, _dev_stream(sb), index, info, a.size // 2, a.size // 4)
    assert st == hs.MONO_INDEX_MISMATCH and o.guards_hold()

    # the stream corrupted inside the range, away from the records' tagged bytes: the decoder's error bits
    blob = index.cpu().numpy()
    pos = [int(blob[64 + 96 * k : 68 + 96 * k].view(np.uint32)[0]) for k in range(info.recordCount)]
    k = next(k for k in range(8, info.recordCount - 1) if pos[k + 1] - pos[k] >= 400)
    bad = bytearray(sa)
    bad[pos[k] + 32 : pos[k] + 32 + 256] = b"\xff" * 256                   # headers of 0xFF claim 2^31 literal bytes
    lo = (k - 2) * 4096
    o, st = _enqueue_one(hs, _dev_stream(bytes(bad)), index, info, lo, 5 * 4096 + 17)
    assert st == hs.MONO_MALFORMED and o.guards_hold()
    # ... and a range that does not reach the corruption is unaffected
    o, st = _enqueue_one(hs, _dev_stream(bytes(bad)), index, info, 0, 4096 * (k - 1))
    assert st == hs.MONO_DONE and torch.equal(o.view.cpu(), torch.from_numpy(a[: 4096 * (k - 1)])) and o.guards_hold()


def test_range_decode_in_a_hip_graph(hs, oracle):
    """Capture a range decode once; replay it after copying other stream bytes and their index (same codec and sizes) into the same buffers."""
    import torch

    key = "rle8_packed_multi"
    codec = CODEC_BY_KEY[key]
    a = oracle.synth(SYNTH_RUNS, 1, 31, 6 << 20)
    b = (a ^ np.uint8(0x5A)).astype(np.uint8)
    sa, sb = oracle.compress(codec, a.tobytes()), oracle.compress(codec, b.tobytes())
    if len(sa) != len(sb):
        pytest.skip("streams of different sizes: not the same launch geometry")
    t = _dev_stream(sa)
    ia, info = hs.mono_index_build(key, t, spacing=1024)
    ib, _ = hs.mono_index_build(key, _dev_stream(sb), spacing=1024)
    assert ia.numel() == ib.numel()
    blobs = {0: ia.cpu(), 1: ib.cpu()}
    index = ia.clone()
    off, n = 1234567, (1 << 20) + 4321
    o, st = _Out(n), _status()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hs.mono_decompress_range_dev_async(t, index, info, off, n, o.view, st)   # warm-up outside the capture
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        hs.mono_decompress_range_dev_async(t, index, info, off, n, o.view, st)
    # (info holds the stream head, which differs between a and b: a replay of b must say so, and b's own info must pass -- the head is
    #  compared on the device, so the captured call keeps a's head)
    for which, stream, data in ((1, sb, b), (0, sa, a), (1, sb, b), (0, sa, a)):
        t[: len(stream)] = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
        index.copy_(blobs[which])
        o.buf.fill_(0xA5)
        st.fill_(0x4D)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        if stream[:16] == sa[:16]:
            assert _word(st) == hs.MONO_DONE
            assert torch.equal(o.view.cpu(), torch.from_numpy(data[off : off + n])) and o.guards_hold()
        else:
            assert _word(st) == hs.MONO_INDEX_MISMATCH and o.untouched()


def test_range_decode_in_a_hip_graph_same_head(hs, oracle):
    """The same with streams whose first 16 bytes agree: every replay decodes the new bytes."""
    import torch

    key = "rle16_sym_packed"
    codec = CODEC_BY_KEY[key]
    a = oracle.synth(SYNTH_RUNS, 2, 41, 6 << 20)
    b = a.copy()
    b[4096:] ^= np.uint8(0x33)
    sa, sb = oracle.compress(codec, a.tobytes()), oracle.compress(codec, b.tobytes())
    if len(sa) != len(sb) or sa[:16] != sb[:16]:
        pytest.skip("streams of different sizes or heads: not the same launch geometry")
    t = _dev_stream(sa)
    ia, info = hs.mono_index_build(key, t, spacing=2048)
    ib, _ = hs.mono_index_build(key, _dev_stream(sb), spacing=2048)
    blobs = {0: ia.cpu(), 1: ib.cpu()}
    index = ia.clone()
    off, n = 777777, 3 << 20
    o, st = _Out(n), _status()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hs.mono_decompress_range_dev_async(t, index, info, off, n, o.view, st)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        hs.mono_decompress_range_dev_async(t, index, info, off, n, o.view, st)
    for which, stream, data in ((1, sb, b), (0, sa, a), (1, sb, b)):
        t[: len(stream)] = torch.frombuffer(bytearray(stream), dtype=torch.uint8).cuda()
        index.copy_(blobs[which])
        o.buf.fill_(0xA5)
        st.fill_(0x4D)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert _word(st) == hs.MONO_DONE
        assert torch.equal(o.view.cpu(), torch.from_numpy(data[off : off + n])) and o.guards_hold()


@pytest.mark.parametrize("key", ["rle8_packed_multi", "rle8_single", "rle128_sym", "rle24_3symlut_byte", "rle48_7symlut_byte_short"])
@pytest.mark.parametrize("block", [4096, 65536, 1 << 20])
def test_container_range_decode(hs, oracle, key, block):
    import torch

    codec = CODEC_BY_KEY[key]
    data = _mixed(oracle, codec.S, 13, (5 << 20) + 4321)
    src = torch.from_numpy(data).cuda()
    container, info = hs.compress(key, src, block_size=block)
    U = data.size
    rng = random.Random(block + len(key))
    ranges = [(0, U), (0, 1), (U - 1, 1), (0, block + 3), (U - block - 3, block + 3), (block - 1, 2)]
    for _ in range(4):                                                    # inside one block
        blk = rng.randrange(info.blockCount - 1)
        a = blk * block + rng.randrange(block - 64)
        ranges.append((a, rng.randrange(1, block * (blk + 1) - a + 1)))
    for _ in range(4):                                                    # across many blocks
        a = rng.randrange(U // 2)
        ranges.append((a, rng.randrange(2 * block, U - a + 1) if U - a > 2 * block else U - a))
    outs = []
    for off, n in ranges:
        o, st = _Out(n), _status()
        hs.decompress_range_dev_async(container, info, off, n, o.view, st)
        outs.append((off, n, o, st))
    torch.cuda.synchronize()
    for off, n, o, st in outs:
        assert _word(st) == hs.MONO_DONE, f"range [{off}, +{n}): status {_word(st)}"
        assert torch.equal(o.view, src[off : off + n]), f"range [{off}, +{n}) differs"
        assert o.guards_hold(), f"range [{off}, +{n}): bytes outside dOut were written"


def test_arguments_are_refused_before_anything_is_enqueued(hs, oracle):
    import torch

    key = "rle32_sym"
    codec = CODEC_BY_KEY[key]
    data = oracle.synth(SYNTH_RUNS, 4, 3, 1 << 20)
    stream = oracle.compress(codec, data.tobytes())
    t = _dev_stream(stream)
    index, info = hs.mono_index_build(key, t, spacing=1024)
    U = data.size
    o, st = _Out(4096), _status()
    for off, n in ((U - 10, 11), (U + 1, 0), (2**40, 1)):                # beyond the end
        with pytest.raises(hs.HsrleError):
            hs.mono_decompress_range_dev_async(t, index, info, off, n, o.view, st)
    with pytest.raises(hs.HsrleError):                                    # output too small
        hs.mono_decompress_range_dev_async(t, index, info, 0, 4097, o.view, st)
    hs.mono_decompress_range_dev_async(t, index, info, 100, 0, o.view, st)   # empty: OK, nothing enqueued
    for spacing in (200, 64, 1 << 21):                                    # spacing: a multiple of 128 in [128, 1 MiB]
        with pytest.raises(hs.HsrleError):
            hs.mono_index_build(key, t, spacing=spacing)
    small = torch.full((hs.mono_index_size(key, U, len(stream), 1024) - 1,), 0x77, dtype=torch.uint8, device="cuda")
    with pytest.raises(hs.HsrleError):                                    # index capacity too small
        hs.mono_index_build(key, t, spacing=1024, index=small)
    with pytest.raises(TypeError):
        hs.mono_decompress_range_dev_async(t, index.cpu(), info, 0, 16, o.view, st)
    container, cinfo = hs.compress(key, torch.from_numpy(data).cuda(), block_size=4096)
    with pytest.raises(hs.HsrleError):
        hs.decompress_range_dev_async(container, cinfo, U - 1, 2, o.view, st)
    with pytest.raises(hs.HsrleError):
        hs.decompress_range_dev_async(container, cinfo, 0, 4097, o.view, st)
    torch.cuda.synchronize()
    assert o.untouched() and bool((st == 0x4D).all())
    assert bool((small == 0x77).all())
