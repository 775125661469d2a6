"""The rle8_sh block container on the GPU (csrc/hsrle_rle8shb.hip.h) against the container built in plain Python (tests/rle8_sh_blocks_testlib.py) from
the sequential models of tests/rle8_sh_testlib.py.  Encode: header, table, payload and pad equal the Python-built container byte for byte, whatever
the number of blocks in flight.  Decode: its own containers, the Python-built ones, block ranges, block streams written from the grammar; a
malformed block (its table entry or its stream) has none of its bytes written while its neighbours are decoded.  Every buffer lies between 0xEE
canaries, every workspace starts as 0xC3 garbage; malformed input is refused by bounds checks, as in test_gpu_rle8_sh.py."""
import struct

import numpy as np
import pytest

import rle8_sh_blocks_testlib as B
import rle8_sh_testlib as T
from mmtf_testlib import video_shaped

pytestmark = pytest.mark.gpu

GUARD = 4096
DONE, MALFORMED, CAPACITY = 0, 1, 2
OK, ERR_FORMAT = 0, 3
BLOCK_SIZES = (128, 1152, 4096)


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    hsrle.rle8_sh_tuning(0, 0, 0)
    hsrle.rle8_sh_blocks_tuning(0)
    yield hsrle
    hsrle.rle8_sh_tuning(0, 0, 0)
    hsrle.rle8_sh_blocks_tuning(0)


@pytest.fixture
def tuned(hs):
    yield hs
    hs.rle8_sh_tuning(0, 0, 0)                                                  # (process-global)
    hs.rle8_sh_blocks_tuning(0)


# ---- inputs ----

def members(n, start=0):
    """n bytes: members of T.input_set() one behind the other."""
    parts, out = list(T.input_set().values()), bytearray()
    k = start
    while len(out) < n:
        out += parts[k % len(parts)]
        k += 7
    return bytes(out[:n])


def straddling_runs(bs, value, length):
    """For every k in 1 .. 14: a run of `length` bytes of `value` that begins k bytes in front of a block edge."""
    out = bytearray()
    for k in range(1, 15):
        piece = T.noise(bs - k, k, avoid=(0x7F, value)) + bytes([value]) * length
        out += piece + T.noise(2 * bs - len(piece), k + 20, avoid=(0x7F, value))
    assert len(out) == 28 * bs
    return bytes(out)


def varied(n):
    q = n // 4
    return (T.short_coded_stretches(q) + T.r_rich(q, 4, 3) + video_shaped(q) + T.noise(n - 3 * q, 6))[:n]


def special_blocks(bs):
    """A block of only 0x7F, a block of random bytes (one raw COPY), a block of another symbol only, then a mix."""
    import random

    return b"\x7F" * bs + random.Random(bs).randbytes(bs) + b"\x11" * bs + members(bs + 9, 3)


# ---- device calls ----

def to_dev(data, offset=0):
    import torch

    t = torch.zeros(len(data) + offset + 64, dtype=torch.uint8, device="cuda")[offset : offset + len(data)]
    t.copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))
    return t


def compress_dev(hs, data, bs, offsets=(0, 0, 0), cap=None):
    """(size word, status word, the out buffer's bytes, 0xEE everywhere outside [0, max(size, `written`))?).  Out buffer: 0xEE, workspace: 0xC3."""
    import torch

    n = len(data)
    cap = hs.rle8_sh_blocks_bound(n, bs) if cap is None else cap
    src = to_dev(data, offsets[0])
    lead = GUARD + offsets[1]
    full = torch.full((lead + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dst = full[lead : lead + cap]
    ws = torch.full((hs.rle8_sh_blocks_workspace_size(0, n, bs) + offsets[2],), 0xC3, dtype=torch.uint8, device="cuda")[offsets[2] :]
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hs.rle8_sh_blocks_compress_dev(src, dst, size, status, ws, block_size=bs)
    torch.cuda.synchronize()
    size, status = int(size.item()), int(status.item())
    host = full.cpu().numpy()
    end = size if status == DONE else cap                                      # (CAPACITY: what lies inside the capacity is unspecified)
    clean = bool((host[:lead] == 0xEE).all() and (host[lead + end :] == 0xEE).all())
    return size, status, host[lead : lead + cap].tobytes(), clean


def check_encode(hs, name, data, bs, offsets=(0, 0, 0)):
    want = B.build(data, bs)
    size, status, out, clean = compress_dev(hs, data, bs, offsets)
    assert (status, size) == (DONE, len(want)), name
    assert out[:64] == want[:64], f"{name}: the header differs"
    nb = B.block_count(len(data), bs)
    assert out[64 : 64 + 8 * (nb + 1)] == want[64 : 64 + 8 * (nb + 1)], f"{name}: the offset table differs"
    assert out[:size] == want, f"{name}: payload or pad differ from the Python-built container"
    assert clean, f"{name}: compress wrote outside [0, totalSize)"
    return want


def info_of(hs, container):
    return hs.rle8_sh_blocks_info(bytes(container))


def decompress_dev(hs, container, first=0, count=None, offsets=(0, 0, 0)):
    """(status word, the output buffer's bytes, canaries on both sides intact?).  Output buffer: 0xEE, workspace: 0xC3 garbage."""
    import torch

    info = info_of(hs, container)
    n, count = info.uncompressedSize, info.blockCount - first if count is None else count
    src = to_dev(container, offsets[0])
    lead = GUARD + offsets[1]
    full = torch.full((lead + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dst = full[lead : lead + n]
    need = hs.rle8_sh_blocks_workspace_size(1, count * info.blockSize, info.blockSize)
    ws = torch.full((need + offsets[2],), 0xC3, dtype=torch.uint8, device="cuda")[offsets[2] :]
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hs.rle8_sh_blocks_decompress_dev(src, info, dst, status, ws, first_block=first, block_count=count)
    torch.cuda.synchronize()
    host = full.cpu().numpy()
    clean = bool((host[:lead] == 0xEE).all() and (host[lead + n :] == 0xEE).all())
    return int(status.item()), host[lead : lead + n].tobytes(), clean


def expected_blocks(container, first=0, count=None):
    """(status, output over 0xEE) by the format's rules, block by block: a bad table entry or a stream the model decoder refuses leaves its range
    untouched."""
    h = B.header(container)
    n, bs, nb = h["uncompressedSize"], h["blockSize"], h["blockCount"]
    off = struct.unpack_from(f"<{nb + 1}Q", container, 64)
    start = 64 + 8 * (nb + 1)
    out, status = bytearray(b"\xEE" * n), DONE
    for i in range(first, nb if count is None else first + count):
        size = min(bs, n - i * bs)
        back = None
        if off[i] <= off[i + 1] <= h["payloadSize"]:
            stream = container[start + off[i] : start + off[i + 1]]
            back = T.model_decompress(stream)
            if back is not None and len(back) != size:
                back = None
        if back is None:
            status = MALFORMED
        else:
            out[i * bs : i * bs + size] = back
    return status, bytes(out)


def check_decode(hs, name, container, first=0, count=None, offsets=(0, 0, 0)):
    want = expected_blocks(container, first, count)
    status, back, clean = decompress_dev(hs, container, first, count, offsets)
    assert status == want[0], name
    assert back == want[1], f"{name}: decode differs"
    assert clean, f"{name}: wrote outside the output"
    return status, back


# ---- encode ----

SHAPES = [(bs, n) for bs in BLOCK_SIZES for n in (1, bs - 1, bs, bs + 1, 3 * bs + 17)]


@pytest.mark.parametrize("bs,n", SHAPES)
def test_compress_gives_the_python_built_container(hs, bs, n):
    data = members(n, bs)
    want = check_encode(hs, f"members {n} / {bs}", data, bs)
    _, streams = B.split(want)
    for i, (s, b) in enumerate(zip(streams, B.blocks_of(data, bs))):
        assert hs.rle8_sh_decompress(s, len(b)) == (len(b), b), f"block {i}: the single-stream decoder"
    assert hs.rle8_sh_blocks_compress_host(data, bs) == (OK, want)
    assert hs.rle8_sh_blocks_decompress_host(want, n) == (OK, data)
    status, back = check_decode(hs, "its own container", want)
    assert (status, back) == (DONE, data)


@pytest.mark.parametrize("blocks", (2, 65, 257))
def test_block_counts_past_a_wave_and_past_a_workgroup(hs, blocks):
    data = varied(blocks * 128 - 41)
    want = check_encode(hs, f"{blocks} blocks", data, 128)
    assert check_decode(hs, f"{blocks} blocks", want) == (DONE, data)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_varied_and_special_blocks(hs, bs):
    for name, data in (("varied", varied(5 * bs + 77)), ("special", special_blocks(bs))):
        want = check_encode(hs, f"{name} / {bs}", data, bs)
        assert check_decode(hs, f"{name} / {bs}", want) == (DONE, data)
    _, streams = B.split(B.build(special_blocks(bs), bs))
    assert len(streams[1]) == bs + (18 if bs > 262 else 15)                   # random bytes: header, one raw COPY (large / small), the terminator


@pytest.mark.parametrize("bs", (128, 1152))
@pytest.mark.parametrize("value,length", ((0x7F, 20), (0x33, 16)))
def test_runs_that_straddle_block_edges(hs, bs, value, length):
    """A run of >= 15 bytes of R (a FILL inside one stream) and a run of >= 10 bytes of another value (a change of R), cut by a block edge at
    every offset 1 .. 14 into the run: each side is decided from the block's own bytes."""
    data = straddling_runs(bs, value, length)
    for k in range(1, 15):
        edge = (2 * (k - 1) + 1) * bs
        assert data[edge - k : edge - k + length] == bytes([value]) * length and data[edge - k - 1] != value
    want = check_encode(hs, f"straddling {value:02x} / {bs}", data, bs)
    assert check_decode(hs, "straddling", want) == (DONE, data)


@pytest.mark.parametrize("offsets", ((1, 3, 5), (3, 17, 1), (17, 1, 3)))
def test_odd_addresses(hs, offsets):
    for bs in BLOCK_SIZES:
        data = varied(3 * bs + 17)
        want = check_encode(hs, f"odd {offsets} / {bs}", data, bs, offsets)
        assert check_decode(hs, f"odd {offsets} / {bs}", want, offsets=offsets) == (DONE, data)
        assert check_decode(hs, f"odd range {offsets} / {bs}", want, 1, 2, offsets)[0] == DONE


# ---- capacity ----

@pytest.mark.parametrize("in_flight", (0, 3))
def test_capacity_one_byte_short(tuned, in_flight):
    """outCapacity = totalSize - 1: CAPACITY, size 0, the magic struck, nothing at or behind outCapacity.  With 3 blocks in flight the first groups
    have written their streams: what lies inside the capacity is unspecified.  (The buffer holds a VALID container from a call before: the strike
    is a write, not an absence.)"""
    tuned.rle8_sh_blocks_tuning(in_flight)
    data = varied(8 * 128 - 3)
    want = B.build(data, 128)
    size, status, out, clean = compress_dev(tuned, data, 128, cap=len(want) - 1)
    assert (size, status) == (0, CAPACITY)
    assert out[:8] != B.MAGIC and clean
    size, status, out, clean = compress_dev(tuned, data, 128, cap=len(want))
    assert (size, status, out, clean) == (len(want), DONE, want, True)
    size, status, out, clean = compress_dev(tuned, data, 128, cap=tuned.rle8_sh_blocks_bound(len(data), 128))
    assert (size, status, out[:size], clean) == (len(want), DONE, want, True)


def test_capacity_strikes_a_magic_that_was_there(hs):
    import torch

    data = varied(8 * 128)
    want = B.build(data, 128)
    cap = len(want) - 1
    src = to_dev(data)
    full = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    full[:cap].copy_(torch.from_numpy(np.frombuffer(want[:cap], dtype=np.uint8).copy()))
    ws = torch.full((hs.rle8_sh_blocks_workspace_size(0, len(data), 128),), 0xC3, dtype=torch.uint8, device="cuda")
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hs.rle8_sh_blocks_compress_dev(src, full[:cap], size, status, ws, block_size=128)
    torch.cuda.synchronize()
    host = full.cpu().numpy()
    assert (int(size.item()), int(status.item())) == (0, CAPACITY)
    assert host[:8].tobytes() != B.MAGIC and (host[cap:] == 0xEE).all()


def test_the_bound_suffices_for_inputs_built_to_grow(hs):
    for name, data in (("marginal_encoded_spans", T.marginal_encoded_spans(1500)), ("raw_blocks_between_changes", T.raw_blocks_between_changes(273 * 40)),
                       ("short_coded_stretches", T.short_coded_stretches(9000))):
        for bs in (1152, 4096):
            want = B.build(data, bs)
            assert len(want) <= hs.rle8_sh_blocks_bound(len(data), bs), name
            check_encode(hs, name, data, bs)


# ---- decode ----

def test_a_block_range_writes_only_its_bytes(hs):
    for bs in BLOCK_SIZES:
        data = varied(3 * bs + 17)
        c = B.build(data, bs)
        status, back = check_decode(hs, "blocks 1 and 2 of 4", c, 1, 2)
        assert status == DONE and back == b"\xEE" * bs + data[bs : 3 * bs] + b"\xEE" * 17
        status, back = check_decode(hs, "the last, short block", c, 3, 1)
        assert status == DONE and back == b"\xEE" * (3 * bs) + data[3 * bs :]


def hand_made_block():
    """128 bytes no encoder writes: a literal that promotes behind S and one behind T, a FILL large through the 32-bit wrap, a gap between body
    and bits."""
    Z, S, Tk = ("Z",), ("S",), ("T",)
    L = lambda v: ("L", v)  # noqa: E731
    tokens = [L(0x21), L(0x21), L(0x30), S, L(0x21), Tk, S, Z, L(0x30), Tk,                 # L(0x21) behind S equals lastOccurred: it promotes
              L(0x40), L(0x40), L(0x50), L(0x50), Tk, L(0x40), Tk, S, Z,                    # L(0x40) behind T equals lastOccurred: it promotes
              ("FILLL", T.wrapped(9), 0x22), Z, Z, ("COPY", T.noise(7, 5)), ("FILL", 91), ("END",)]
    stream = T.write_stream(128, tokens, gap=5)
    want = T.model_decompress(stream)
    assert want is not None and len(want) == 128
    return stream, want


def test_a_hand_made_middle_block_decodes_as_the_model_does(tuned):
    data = varied(3 * 128)
    stream, middle = hand_made_block()
    _, streams = B.split(B.build(data, 128))
    c = B.from_streams([streams[0], stream, streams[2]], 3 * 128, 128)
    for serial in (0, 1):
        tuned.rle8_sh_tuning(0, 0, serial)
        assert check_decode(tuned, "hand-made middle block", c) == (DONE, data[:128] + middle + data[256:])
    assert tuned.rle8_sh_blocks_decompress_host(c, 3 * 128) == (OK, data[:128] + middle + data[256:])


GRAMMAR = T.grammar_streams()


@pytest.mark.parametrize("name", list(GRAMMAR))
def test_grammar_written_streams_as_one_block_containers(hs, name):
    stream = GRAMMAR[name]
    want = T.model_decompress(stream)
    assert want is not None
    bs = (len(want) + 127) // 128 * 128
    c = B.from_streams([stream], len(want), bs)
    assert check_decode(hs, name, c) == (DONE, want)


# ---- malformed ----

def test_malformed_streams_as_one_block_containers(hs):
    good, bad = T.malformed_streams()
    assert check_decode(hs, "good", B.from_streams([good], 30, 128)) == (DONE, T.model_decompress(good))
    for name, (n, stream) in bad.items():
        c = B.from_streams([stream], n, (n + 127) // 128 * 128)
        status, out, clean = decompress_dev(hs, c)
        assert status == MALFORMED, name
        assert clean and out == b"\xEE" * n, f"{name}: the output or the canary around it was touched"
        assert hs.rle8_sh_blocks_decompress_host(c, n + 64) == (ERR_FORMAT, b""), name


def test_a_cut_middle_stream_leaves_its_neighbours_whole(hs):
    data = varied(3 * 1152)
    _, streams = B.split(B.build(data, 1152))
    c = B.from_streams([streams[0], streams[1][:-1], streams[2]], len(data), 1152)           # (the table is consistent: the stream is a byte short)
    status, out = check_decode(hs, "cut middle stream", c)
    assert status == MALFORMED
    assert out == data[:1152] + b"\xEE" * 1152 + data[2304:]


def test_bad_table_entries(hs):
    data = varied(3 * 128 + 17)
    _, streams = B.split(B.build(data, 128))
    sizes = [len(s) for s in streams]
    o = [0, sizes[0], sizes[0] + sizes[1], sum(sizes[:3]), sum(sizes)]
    backwards = list(o)
    backwards[2] = o[1] - 1                                                  # entry 1 runs backwards; entry 2 then begins inside stream 0
    c = B.from_streams(streams, len(data), 128, offsets=backwards)
    status, out = check_decode(hs, "an entry that runs backwards", c)
    assert status == MALFORMED and out[:128] == data[:128] and out[128:384] == b"\xEE" * 256 and out[384:] == data[384:]
    beyond = list(o)
    beyond[4] = o[4] + 5                                                     # the last entry passes payloadSize
    c = B.from_streams(streams, len(data), 128, offsets=beyond)
    status, out = check_decode(hs, "an entry that passes payloadSize", c)
    assert status == MALFORMED and out == data[:384] + b"\xEE" * 17
    huge = list(o)
    huge[1] = (1 << 64) - 8
    c = B.from_streams(streams, len(data), 128, offsets=huge)
    status, out = check_decode(hs, "an entry near 2^64", c)
    assert status == MALFORMED and out == b"\xEE" * 256 + data[256:]


# ---- tuning ----

def test_every_tuning_value_gives_the_same_bytes(tuned):
    data8, data65 = varied(8 * 128 - 3), varied(65 * 128 - 9)
    stream, middle = hand_made_block()
    _, s8 = B.split(B.build(data8, 128))
    hand = B.from_streams(s8[:3] + [stream] + s8[4:], len(data8), 128)
    cut = B.from_streams(s8[:5] + [s8[5][:-1]] + s8[6:], len(data8), 128)
    for in_flight, blocks_data in ((1, data8), (3, data8), (0, data8), (64, data65), (0, data65)):
        tuned.rle8_sh_blocks_tuning(in_flight)
        want = check_encode(tuned, f"in flight {in_flight}", blocks_data, 128)
        assert check_decode(tuned, f"in flight {in_flight}", want) == (DONE, blocks_data)
        assert check_decode(tuned, f"in flight {in_flight}: hand-made", hand) == (DONE, data8[:384] + middle + data8[512:])
        status, out = check_decode(tuned, f"in flight {in_flight}: cut", cut)
        assert status == MALFORMED and out == data8[:640] + b"\xEE" * 128 + data8[768:]
    tuned.rle8_sh_blocks_tuning(3)
    big = varied(3 * 4096 + 17)
    for stretch, window, serial in ((1, 64, 0), (7, 80, 1), (4096, 1008, 0), (0, 0, 1)):
        tuned.rle8_sh_tuning(stretch, window, serial)
        for bs, d in ((128, data8), (4096, big)):
            assert check_decode(tuned, f"tuning {stretch} {window} {serial}", B.build(d, bs)) == (DONE, d)
        assert check_decode(tuned, "tuning: hand-made", hand) == (DONE, data8[:384] + middle + data8[512:])
        assert check_decode(tuned, "tuning: cut", cut)[0] == MALFORMED


# ---- graph ----

def test_graph_capture_and_replay(tuned):
    """Compress then decompress (a linear chain) captured once on a side stream, two groups each, and replayed on new bytes with the workspaces
    refilled with garbage.  (The container's sizes are part of the captured decode call: the replays' inputs give containers of the same size.)"""
    import torch

    tuned.rle8_sh_blocks_tuning(3)
    n, bs = 700, 128
    inputs = [bytes([a]) * 20 + T.noise(300, a, avoid=(0x7F,)) + b"\x7F" * 80 + T.noise(300, a + 9, avoid=(0x7F,)) for a in (1, 2, 3)]
    wants = [B.build(d, bs) for d in inputs]
    assert len({len(c) for c in wants}) == 1
    total, cap = len(wants[0]), tuned.rle8_sh_blocks_bound(n, bs)
    info = info_of(tuned, wants[0])
    src = to_dev(inputs[0])
    enc = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dec = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    ws1 = torch.full((tuned.rle8_sh_blocks_workspace_size(0, n, bs),), 0xC3, dtype=torch.uint8, device="cuda")
    ws2 = torch.full((tuned.rle8_sh_blocks_workspace_size(1, n, bs),), 0xC3, dtype=torch.uint8, device="cuda")
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    words = torch.full((2,), -1, dtype=torch.int32, device="cuda")

    def both(stream):
        tuned.rle8_sh_blocks_compress_dev(src, enc[:cap], size, words[0:1], ws1, block_size=bs, stream=stream)
        tuned.rle8_sh_blocks_decompress_dev(enc[:total], info, dec[:n], words[1:2], ws2, stream=stream)

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        both(side)                                                           # warm-up outside the capture (module load)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        both(side)
    for data, want in zip(inputs[1:], wants[1:]):
        src.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
        enc.fill_(0xEE)
        dec.fill_(0xEE)
        ws1.fill_(0x5A)
        ws2.fill_(0xA5)
        size.fill_(-1)
        words.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        e, d = enc.cpu().numpy(), dec.cpu().numpy()
        assert (int(size.item()), [int(x) for x in words.cpu().numpy()]) == (total, [DONE, DONE])
        assert e[:total].tobytes() == want
        assert d[:n].tobytes() == data
        assert (e[total:] == 0xEE).all() and (d[n:] == 0xEE).all()
