"""mmtf128 / mmtf256 / bitmmtf8 / bitmmtf16 on the GPU (csrc/hsrle_mmtf.hip.h) against the sequential definition (tests/mmtf_testlib.py) and, where
it is present, the compiled reference.  The device entry point over sizes that cross every border (no row, one row, a tail, 16-row tiles, many
segments) and segment / chunk lengths 1, 2, 7, 64 and the library's own; byte-exact output, nothing written at or behind `size`, a workspace that
starts as garbage, any alignment, a captured HIP graph replayed on new bytes, the ten host-pointer functions, and the transform in one stream with
the block codec."""
import ctypes

import numpy as np
import pytest

import mmtf_testlib as mt

pytestmark = pytest.mark.gpu

TUNINGS = [1, 2, 7, 64, 0]
GUARD = 4096
_MODEL = {}


def want(transform, decode, data):
    key = (transform, decode, data)
    if key not in _MODEL:
        _MODEL[key] = mt.model(transform, decode, data)
    return _MODEL[key]


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    hsrle.mmtf_tuning(0)
    yield hsrle
    hsrle.mmtf_tuning(0)


@pytest.fixture
def tuned(hs):
    yield hs
    hs.mmtf_tuning(0)                                                        # (process-global)


@pytest.fixture(scope="module")
def ref():
    return mt.MmtfReference() if mt.MmtfReference.available() else None


def run_dev(hs, transform, decode, data, src_offset=0, dst_offset=0, stream=None):
    """One enqueue on fresh buffers: (output bytes, guard untouched?).  The output buffer is `size + GUARD` bytes of 0xEE, the workspace 0xC3."""
    import torch

    n = len(data)
    src = torch.zeros(n + src_offset + 64, dtype=torch.uint8, device="cuda")[src_offset : src_offset + n]
    if n:
        src.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
    full = torch.full((dst_offset + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dst = full[dst_offset:]
    ws = torch.full((max(hs.mmtf_workspace_size(transform, n), 1),), 0xC3, dtype=torch.uint8, device="cuda")
    hs.mmtf_dev(transform, decode, src, dst, ws, stream=stream)
    torch.cuda.synchronize()
    host = full.cpu().numpy()
    clean = bool((host[:dst_offset] == 0xEE).all() and (host[dst_offset + n :] == 0xEE).all())
    return host[dst_offset : dst_offset + n].tobytes(), clean


def inputs_for(transform):
    W = mt.WIDTH[transform]
    out = [(f"n{n}_a5", mt.random_bytes(n, 5, 41)) for n in mt.sizes_for(W)]
    for n in (64 * W + 5, 4096):
        out += [(f"n{n}_one_symbol", bytes([7]) * n), (f"n{n}_a2", mt.random_bytes(n, 2, 43)), (f"n{n}_a256", mt.random_bytes(n, 256, 47))]
    out.append(("all_symbols_per_column_4096", mt.every_symbol_per_column(4096, W)))
    out.append(("all_symbols_per_column_big", mt.every_symbol_per_column(65536 + W + 3, W)))
    out.append(("late_symbols_some_columns", mt.late_symbols_in_some_columns(64 * W + 5, W, 7)))
    out.append(("late_symbols_some_columns_64", mt.late_symbols_in_some_columns(300 * W + 9, W, 64)))
    return out


@pytest.mark.parametrize("tuning", TUNINGS)
@pytest.mark.parametrize("decode", (0, 1))
@pytest.mark.parametrize("transform", mt.TRANSFORMS)
def test_device_entry_point(tuned, transform, decode, tuning):
    """every size x every input kind; decode takes the same arbitrary bytes (any byte string is a valid input of every decode)"""
    tuned.mmtf_tuning(tuning)
    for name, data in inputs_for(transform):
        got, clean = run_dev(tuned, transform, decode, data)
        assert got == want(transform, decode, data), f"{mt.function_name(transform, decode)} {name} tuning {tuning}"
        assert clean, f"{name}: bytes outside [0, size) were written"


@pytest.mark.parametrize("tuning", (7, 0))
@pytest.mark.parametrize("transform", mt.TRANSFORMS)
def test_round_trip(tuned, transform, tuning):
    tuned.mmtf_tuning(tuning)
    W = mt.WIDTH[transform]
    for data in (mt.random_bytes(64 * W + 5, 256, 53), mt.random_bytes(65536 + W + 3, 40, 59), mt.every_symbol_per_column(4096 + 3, W)):
        enc, _ = run_dev(tuned, transform, 0, data)
        dec, _ = run_dev(tuned, transform, 1, enc)
        assert dec == data


@pytest.mark.parametrize("offsets", ((1, 3), (3, 17), (17, 1)))
@pytest.mark.parametrize("transform", mt.TRANSFORMS)
def test_any_alignment(tuned, transform, offsets):
    W = mt.WIDTH[transform]
    for tuning in (7, 0):
        tuned.mmtf_tuning(tuning)
        for data in (mt.random_bytes(64 * W + 5, 5, 61), mt.random_bytes(65536 + W + 3, 256, 67)):
            for decode in (0, 1):
                got, clean = run_dev(tuned, transform, decode, data, src_offset=offsets[0], dst_offset=offsets[1])
                assert got == want(transform, decode, data), (offsets, tuning, decode, len(data))
                assert clean


@pytest.mark.parametrize("transform", mt.TRANSFORMS)
def test_size_zero_and_errors(hs, transform):
    import torch

    L = hs.lib()
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda")
    ws = torch.full((hs.mmtf_workspace_size(transform, 4096),), 0xC3, dtype=torch.uint8, device="cuda")
    sp = hs._stream_ptr()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for decode in (0, 1):
        assert L.hsrle_mmtf_dev_async(transform, decode, p(src), 0, p(dst), p(ws), ws.numel(), sp) == hs.OK
        torch.cuda.synchronize()
        assert bool((dst == 0xEE).all()), "size 0 wrote to the output"
        assert L.hsrle_mmtf_dev_async(transform, decode, p(src), 4096, p(dst), p(ws), hs.mmtf_workspace_size(transform, 4096) - 1, sp) == hs.ERR_CAPACITY
        assert L.hsrle_mmtf_dev_async(transform, decode, p(src), 4096, p(src), p(ws), ws.numel(), sp) == hs.ERR_ARGUMENT
        assert L.hsrle_mmtf_dev_async(transform, decode, p(src), 2048, ctypes.c_void_p(src.data_ptr() + 2047), p(ws), ws.numel(), sp) == hs.ERR_ARGUMENT
        assert L.hsrle_mmtf_dev_async(4, decode, p(src), 4096, p(dst), p(ws), ws.numel(), sp) == hs.ERR_ARGUMENT
        assert L.hsrle_mmtf_dev_async(transform, decode, None, 4096, p(dst), p(ws), ws.numel(), sp) == hs.ERR_ARGUMENT
    torch.cuda.synchronize()
    assert bool((dst == 0xEE).all()), "a refused call wrote to the output"


@pytest.mark.parametrize("decode", (0, 1))
@pytest.mark.parametrize("transform", (mt.MMTF128, mt.MMTF256))
def test_one_mib_video_shaped_at_the_librarys_tuning(hs, ref, transform, decode):
    """many tiles per segment, many segments, the library's own segment length; against the compiled reference when present, else the model"""
    hs.mmtf_tuning(0)
    n = 1 << 20
    plain = hs.synth(hs.SYNTH_VIDEO, 1, 9, n, device="cuda").cpu().numpy().tobytes()
    # the decode's input: the encoded form of the same bytes (ranks of a video-shaped input), from the reference / the model
    def truth(d, data):
        if ref is not None:
            rc, out = ref.run(transform, d, data)
            assert rc == len(data)
            return out
        return mt.model(transform, d, data)

    data = truth(0, plain) if decode else plain
    got, clean = run_dev(hs, transform, decode, data)
    assert got == truth(decode, data)
    assert clean
    if decode:
        assert got == plain


def test_graph_capture_and_replay(hs):
    """One mmtf128 encode and one decode, captured once (one linear chain on a side stream) and replayed twice on new input bytes, the workspace
    refilled with garbage before each replay."""
    import torch

    hs.mmtf_tuning(0)
    T, n = mt.MMTF128, 65536 + 16 + 3
    inputs = [mt.random_bytes(n, 5, 71), mt.random_bytes(n, 256, 73), mt.every_symbol_per_column(n, 16)]
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    enc = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dec = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    ws1 = torch.full((hs.mmtf_workspace_size(T, n),), 0xC3, dtype=torch.uint8, device="cuda")
    ws2 = torch.full((hs.mmtf_workspace_size(T, n),), 0xC3, dtype=torch.uint8, device="cuda")
    src.copy_(torch.from_numpy(np.frombuffer(inputs[0], dtype=np.uint8).copy()))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        hs.mmtf_dev(T, 0, src, enc, ws1, stream=side)                        # warm-up outside the capture (module load)
        hs.mmtf_dev(T, 1, enc[:n], dec, ws2, stream=side)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        hs.mmtf_dev(T, 0, src, enc, ws1, stream=side)
        hs.mmtf_dev(T, 1, enc[:n], dec, ws2, stream=side)
    for data in (inputs[1], inputs[2]):
        src.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
        enc.fill_(0xEE)
        dec.fill_(0xEE)
        ws1.fill_(0x5A)
        ws2.fill_(0xA5)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        e, d = enc.cpu().numpy(), dec.cpu().numpy()
        assert e[:n].tobytes() == want(T, 0, data)
        assert d[:n].tobytes() == data
        assert (e[n:] == 0xEE).all() and (d[n:] == 0xEE).all()


@pytest.mark.parametrize("transform", mt.TRANSFORMS)
def test_drop_in_functions(hs, ref, transform):
    """the host-pointer functions behind the reference's names: bytes and return values"""
    hs.mmtf_tuning(0)
    W = mt.WIDTH[transform]
    assert hs.mmtf_bounds(12345) == 12345 and hs.bitmmtf_bounds(12345) == 12345
    for decode in (0, 1):
        f = getattr(hs, mt.function_name(transform, decode))
        for n in mt.sizes_for(W):
            data = mt.random_bytes(n, 40, 79)
            rc, out = f(data)
            assert rc == n
            assert out == want(transform, decode, data), (n, decode)
            if ref is not None:
                rrc, rout = ref.run(transform, decode, data)
                assert (rrc, rout) == (rc, out)
        assert f(b"")[0] == 0                                               # returns inSize
        assert f(bytes(32), out_cap=31)[0] == 0                             # inSize > outSize
        if ref is not None:
            assert ref.run(transform, decode, b"")[0] == 0 and ref.run(transform, decode, bytes(32), out_size=31)[0] == 0


def test_composes_with_the_block_codec_on_one_stream(hs):
    """mmtf128 encode -> rle8_packed_multi compress -> decompress -> mmtf128 decode, enqueued on one stream with no host read in between, gives back
    a 256 KiB video-shaped input.  The container's header fields are remembered from an earlier compression of the same bytes (they are a function
    of the input), as include/hsrle.h allows for hsrle_decompress_dev_async."""
    import torch

    hs.mmtf_tuning(0)
    T, n, key, block = mt.MMTF128, 256 << 10, "rle8_packed_multi", 4096
    src = hs.synth(hs.SYNTH_VIDEO, 1, 21, n, device="cuda")
    ranks = torch.empty(n, dtype=torch.uint8, device="cuda")
    ws = torch.full((hs.mmtf_workspace_size(T, n),), 0xC3, dtype=torch.uint8, device="cuda")
    hs.mmtf_dev(T, 0, src, ranks, ws)
    _, info = hs.compress(key, ranks, block_size=block)                      # (reads the header: this is the rehearsal, not the chain)
    torch.cuda.synchronize()

    side = torch.cuda.Stream()
    ranks.fill_(0xEE)
    container = torch.full((hs.container_bound(n, block),), 0xEE, dtype=torch.uint8, device="cuda")
    cws = torch.full((hs.workspace_size(n, block),), 0xC3, dtype=torch.uint8, device="cuda")
    ranks2 = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    back = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    ws.fill_(0x3C)
    ws2 = torch.full((hs.mmtf_workspace_size(T, n),), 0xC3, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")             # (the block decode ORs error bits into it: the caller clears it)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        hs.mmtf_dev(T, 0, src, ranks, ws, stream=side)
        hs.compress_async(key, ranks, container, block_size=block, workspace=cws, stream=side)
        hs.decompress_async(container, info, ranks2, status=status, stream=side)
        hs.mmtf_dev(T, 1, ranks2, back, ws2, stream=side)
    side.synchronize()
    assert int(status.item()) == 0
    host = back.cpu().numpy()
    assert host[:n].tobytes() == src.cpu().numpy().tobytes()
    assert (host[n:] == 0xEE).all()
    assert hs.container_info(container).totalSize == info.totalSize
