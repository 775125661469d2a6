"""The rle8_mmtf128 block container on the GPU (csrc/hsrle_rle8mmtfb.hip.h) against the container built in plain Python (tests/rle8_mmtf_blocks_testlib.py)
from the sequential model of tests/rle8_mmtf_testlib.py.  Encode: header, table, payload and pad equal the Python-built container byte for byte,
whatever the blocks in flight and the rows per span.  The inputs are made from the PACKETS every block shall produce (the inverse mmtf of chosen rank
rows, block by block: the lists restart at every block), so every header form, width, group remainder and edge is hit by name, in the first, a middle
and the last block.  Decode: its own containers, the Python-built ones, block ranges, block streams written from the grammar; a malformed block (its
table entry or its stream) has none of its bytes written while its neighbours are decoded.  Every buffer lies between 0xEE canaries, every workspace
starts as 0xC3 garbage; malformed input is refused by bounds checks, as in test_gpu_rle8_mmtf.py."""
import random
import struct

import numpy as np
import pytest

import rle8_mmtf_blocks_testlib as B
import rle8_mmtf_testlib as T
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
    hsrle.rle8_mmtf_tuning(0)
    hsrle.rle8_mmtf128_blocks_tuning(0)
    yield hsrle
    hsrle.rle8_mmtf_tuning(0)
    hsrle.rle8_mmtf128_blocks_tuning(0)


@pytest.fixture
def tuned(hs):
    yield hs
    hs.rle8_mmtf_tuning(0)                                                      # (process-global)
    hs.rle8_mmtf128_blocks_tuning(0)


# ---- inputs ----

def varied(n, seed=0):
    """Runs over a small alphabet, video-shaped bytes, a large alphabet, random bytes: every packet kind and width somewhere."""
    q = n // 4
    return (T.random_alphabet(q, 3, 4 + seed, run=3) + video_shaped(q, seed + 3) + T.random_alphabet(q, 40, 5 + seed) + random.Random(n + seed).randbytes(n - 3 * q))[:n]


def noise(n, seed, avoid):
    rng = random.Random(seed)
    return bytes(rng.choice([v for v in range(256) if v != avoid]) for _ in range(n))


def filler(R):
    return [("copy", R // 2, 100), ("rle", R - R // 2, 3)]


def shapes(bs):
    """name -> the packets of ONE block of bs / 16 rows."""
    R = bs // 16
    out = {}
    for top, name, counts in ((3, "2bit", (3, 4, 5)), (7, "3bit", (5, 6, 7)), (15, "4bit", (1, 2, 3)), (255, "8bit", (1, 2))):
        for k in counts:
            if 2 * k + 2 <= R:
                out[f"{name}_{k}_rows"] = [("copy", k, top), ("rle", 1, 0), ("copy", k, top), ("rle", R - 2 * k - 1, 2)]          # ends on an RLE
            else:
                out[f"{name}_{k}_rows"] = [("copy", k, top), ("rle", R - k, 2)]
            out[f"{name}_{k}_rows_last"] = [("rle", R - k, 1), ("copy", k, top)]                                                  # a group that ends at the block's last row
    out["one_uniform_run"] = [("rle", R, 5)]
    out["ends_on_copy"] = [("rle", 3, 0), ("copy", R - 3, 40)]
    out["ends_on_rle"] = [("copy", 2, 40), ("rle", R - 2, 0)]
    out["adjacent_rles"] = [("rle", 1, 0), ("rle", 1, 1), ("rle", 2, 0), ("rle", R - 5, 200), ("rle", 1, 255)]
    if bs == 4096:
        out["copy_31_32_rle_127"] = [("copy", 31, 200), ("rle", 1, 0), ("copy", 32, 200), ("rle", 127, 1), ("copy", 1, 9), ("rle", 64, 0)]
        out["rle_128_copy_32_31"] = [("rle", 128, 1), ("copy", 32, 3), ("rle", 1, 0), ("copy", 31, 7), ("rle", 64, 2)]
        out["one_long_copy"] = [("copy", 256, 255)]
        out["one_long_rle"] = [("rle", 256, 0)]
    if bs == 1152:
        out["2bit_group_across_row_64"] = [("rle", 61, 0), ("copy", 11, 3)]                  # the group of rows 61 .. 64
        out["3bit_group_across_row_64"] = [("rle", 59, 1), ("copy", 13, 7)]                  # rows 59 .. 64
        out["4bit_pair_across_row_64"] = [("rle", 1, 0), ("copy", 71, 15)]                   # rows 63, 64
        out["8bit_across_row_64"] = [("copy", 72, 255)]
        out["rle_across_row_64"] = [("copy", 60, 15), ("rle", 12, 7)]
    for name, spec in out.items():
        assert sum(c for _, c, _ in spec) == R, name
    return out


def placed(bs, spec, seed):
    """The shape in the first, a middle and the last block of five."""
    R = bs // 16
    return B.data_from_block_specs([spec, filler(R), spec, filler(R), spec], bs, seed=seed)


def straddling_runs(bs, value=0x33, length=118):
    """For k = 1 .. 15 bytes and 1 .. 3 rows: a run of `length` bytes of one value that begins k bytes in front of a block edge."""
    out = bytearray()
    ks = list(range(1, 16)) + [16, 32, 48]
    for k in ks:
        piece = noise(bs - k, k, value) + bytes([value]) * length
        out += piece + noise(2 * bs - len(piece), k + 20, value)
    assert len(out) == 2 * len(ks) * bs
    return bytes(out), ks


# ---- device calls ----

def to_dev(data, offset=0):
    import torch

    t = torch.zeros(len(data) + offset + 64, dtype=torch.uint8, device="cuda")[offset : offset + len(data)]
    t.copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))
    return t


def compress_dev(hs, data, bs, offsets=(0, 0, 0), cap=None, before=None):
    """(size word, status word, the out buffer's bytes, 0xEE everywhere outside [0, max(size, `written`))?).  Out buffer: 0xEE (or `before`),
    workspace: 0xC3."""
    import torch

    n = len(data)
    cap = hs.rle8_mmtf128_blocks_bound(n, bs) if cap is None else cap
    src = to_dev(data, offsets[0])
    lead = GUARD + offsets[1]
    full = torch.full((lead + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dst = full[lead : lead + cap]
    if before is not None:
        dst[: len(before)].copy_(torch.from_numpy(np.frombuffer(bytes(before), dtype=np.uint8).copy()))
    ws = torch.full((hs.rle8_mmtf128_blocks_workspace_size(0, n, bs) + offsets[2],), 0xC3, dtype=torch.uint8, device="cuda")[offsets[2] :]
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hs.rle8_mmtf128_blocks_compress_dev(src, dst, size, status, ws, block_size=bs)
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
    table = 64 + 8 * (nb + 1)
    assert out[64:table] == want[64:table], f"{name}: the offset table differs"
    assert out[table : size - 32] == want[table:-32], f"{name}: the payload differs from the Python-built block streams"
    assert out[size - 32 : size] == bytes(32), f"{name}: the pad"
    assert out[:size] == want, name
    assert clean, f"{name}: compress wrote outside [0, totalSize)"
    return want


def info_of(hs, container):
    return hs.rle8_mmtf128_blocks_info(bytes(container))


def decompress_dev(hs, container, first=0, count=None, offsets=(0, 0, 0)):
    """(status word, the output buffer's bytes, canaries on both sides intact?).  Output buffer: 0xEE, workspace: 0xC3 garbage."""
    import torch

    info = info_of(hs, container)
    n, count = info.uncompressedSize, info.blockCount - first if count is None else count
    src = to_dev(container, offsets[0])
    lead = GUARD + offsets[1]
    full = torch.full((lead + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dst = full[lead : lead + n]
    need = hs.rle8_mmtf128_blocks_workspace_size(1, count * info.blockSize, info.blockSize)
    ws = torch.full((need + offsets[2],), 0xC3, dtype=torch.uint8, device="cuda")[offsets[2] :]
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hs.rle8_mmtf128_blocks_decompress_dev(src, info, dst, status, ws, first_block=first, block_count=count)
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
            back = T.model_decompress(container[start + off[i] : start + off[i + 1]])
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

SHAPES = [(bs, n) for bs in BLOCK_SIZES for n in (1, 15, 16, 17, bs - 1, bs, bs + 1, bs + 5, 3 * bs + 17)]


@pytest.mark.parametrize("bs,n", SHAPES)
def test_compress_gives_the_python_built_container(hs, bs, n):
    data = varied(n, bs)
    want = check_encode(hs, f"varied {n} / {bs}", data, bs)
    _, streams = B.split(want)
    for i, (s, b) in enumerate(zip(streams, B.blocks_of(data, bs))):
        assert hs.rle8_mmtf128_decompress(s, len(b)) == (len(b), b), f"block {i}: the single-stream decoder"
    assert hs.rle8_mmtf128_blocks_compress_host(data, bs) == (OK, want)
    assert hs.rle8_mmtf128_blocks_decompress_host(want, n) == (OK, data)
    assert check_decode(hs, "its own container", want) == (DONE, data)


@pytest.mark.parametrize("blocks", (1, 3, 4, 5, 65, 257))
def test_block_counts_past_a_waves_four_blocks_a_wave_and_a_workgroup(hs, blocks):
    data = varied(blocks * 128 - 41, blocks)
    want = check_encode(hs, f"{blocks} blocks", data, 128)
    assert check_decode(hs, f"{blocks} blocks", want) == (DONE, data)


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_every_packet_shape_in_the_first_a_middle_and_the_last_block(hs, bs):
    R = bs // 16
    for k, (name, spec) in enumerate(shapes(bs).items()):
        data = placed(bs, spec, seed=7 * k + 1)
        want = check_encode(hs, f"{name} / {bs}", data, bs)
        _, streams = B.split(want)
        assert T.structure(T.parse_stream(streams[2])[1]) == T.local_rule_packets(b"".join(T.rows_from_spec(spec, 7 * k + 3))), name   # the packets asked for
        assert check_decode(hs, f"{name} / {bs}", want) == (DONE, data)
    # one uniform run: the first COPY 0x06, one RLE, then a null COPY and the null RLE
    _, streams = B.split(B.build(placed(bs, [("rle", R, 5)], 1), bs))
    rle = bytes([R << 1, 5]) if R < 128 else struct.pack("<IB", R << 1 | 1, 5)
    assert streams[0] == streams[4] == struct.pack("<II", bs, 8 + 1 + len(rle) + 2) + b"\x06" + rle + b"\x00\x00"


def test_a_short_last_block_with_rows_and_tail_ranks(hs):
    for bs in BLOCK_SIZES:
        R = bs // 16
        data = B.data_from_block_specs([filler(R), [("copy", 3, 7), ("rle", 2, 1)]], bs, tail=b"\x05\x01\x00", seed=bs)
        assert len(data) == bs + 83
        want = check_encode(hs, f"short last block / {bs}", data, bs)
        assert check_decode(hs, f"short last block / {bs}", want) == (DONE, data)


@pytest.mark.parametrize("bs", (128, 1152))
def test_a_uniform_run_across_a_block_edge_restarts_from_identity_lists(hs, bs):
    """A run of one byte value cut by a block edge 1 .. 15 bytes and 1 .. 3 rows into the run: behind the edge the value is a NEW symbol of identity
    lists (rank = the value itself in row 0, then rank 0), whatever ranks it had in front of the edge."""
    data, ks = straddling_runs(bs)
    for i, k in enumerate(ks):
        edge = (2 * i + 1) * bs
        assert data[edge - k : edge - k + 118] == b"\x33" * 118 and data[edge - k - 1] != 0x33
    want = check_encode(hs, f"straddling / {bs}", data, bs)
    _, streams = B.split(want)
    for i in range(len(ks)):
        _, packets, ranks = T.parse_stream(streams[2 * i + 1])
        assert ranks[:16] == b"\x33" * 16 and ranks[16:48] == bytes(32), i                  # row 0: the value itself; rows 1, 2: rank 0
        assert T.structure(packets)[:4] == [("copy", 0, None), ("rle", 1, 0x33), ("copy", 0, None), ("rle", (118 - ks[i]) // 16 - 1, 0)], i
    assert check_decode(hs, "straddling", want) == (DONE, data)


@pytest.mark.parametrize("offsets", ((1, 3, 5), (3, 17, 1), (17, 1, 3)))
def test_odd_addresses(hs, offsets):
    for bs in BLOCK_SIZES:
        data = varied(3 * bs + 17, 2)
        want = check_encode(hs, f"odd {offsets} / {bs}", data, bs, offsets)
        assert check_decode(hs, f"odd {offsets} / {bs}", want, offsets=offsets) == (DONE, data)
        assert check_decode(hs, f"odd range {offsets} / {bs}", want, 1, 2, offsets)[0] == DONE


# ---- capacity ----

@pytest.mark.parametrize("in_flight", (0, 3))
def test_capacity_one_byte_short(tuned, in_flight):
    """outCapacity = totalSize - 1: CAPACITY, size 0, the magic struck -- over a VALID container from a call before: the strike is a write, not an
    absence --, nothing at or behind outCapacity.  With 3 blocks in flight the first groups have written their streams: what lies inside the capacity
    is unspecified.  Exactly totalSize bytes and exactly the bound both succeed."""
    tuned.rle8_mmtf128_blocks_tuning(in_flight)
    data = varied(8 * 128 - 3, 1)
    want = B.build(data, 128)
    size, status, out, clean = compress_dev(tuned, data, 128, cap=len(want) - 1, before=want[:-1])
    assert (size, status) == (0, CAPACITY)
    assert out[:8] != B.MAGIC and clean
    size, status, out, clean = compress_dev(tuned, data, 128, cap=len(want))
    assert (size, status, out, clean) == (len(want), DONE, want, True)
    size, status, out, clean = compress_dev(tuned, data, 128, cap=tuned.rle8_mmtf128_blocks_bound(len(data), 128))
    assert (size, status, out[:size], clean) == (len(want), DONE, want, True)


def test_the_bound_is_reached_by_incompressible_blocks(hs):
    for bs in (1152, 4096):
        data = B.data_from_block_specs([[("copy", bs // 16, 255)]] * 3, bs)
        want = check_encode(hs, f"incompressible / {bs}", data, bs)
        assert len(want) == hs.rle8_mmtf128_blocks_bound(len(data), bs)
        assert check_decode(hs, f"incompressible / {bs}", want) == (DONE, data)


# ---- decode ----

def test_a_block_range_writes_only_its_bytes(hs):
    for bs in BLOCK_SIZES:
        data = varied(3 * bs + 17, 3)
        c = B.build(data, bs)
        status, back = check_decode(hs, "blocks 1 and 2 of 4", c, 1, 2)
        assert status == DONE and back == b"\xEE" * bs + data[bs : 3 * bs] + b"\xEE" * 17
        status, back = check_decode(hs, "the last, short block", c, 3, 1)
        assert status == DONE and back == b"\xEE" * (3 * bs) + data[3 * bs :]


def grammar_streams(middle):
    """Legal streams no encoder writes (the shapes of test_gpu_rle8_mmtf.py).  middle: made to fill a block -- an RLE packet pads the rows to a
    multiple of 8 (a block size is a multiple of 128 bytes) and there is no tail.  name -> (uncompressed size, stream)."""
    rng = random.Random(21)
    null = ("copy", [], 0, False)
    shapes = {}                                                                 # name -> (rows, packets up to a last COPY, the terminator, tail ranks)
    for code in range(4):
        # a first COPY of no rows with each flag value; a null COPY in long form; the terminator in long form
        shapes[f"first_null_copy_code{code}"] = (3, [("copy", [], code, False), ("rle", 2, 5, False), ("copy", [], code, True), ("rle", 1, 5, False), null], ("rle", 0, None, True), b"")
        # 4-byte COPY headers with counts below 32, rows narrower than their width
        rows = T.literal_rows(7, 3, rng)
        shapes[f"long_copy_header_code{code}"] = (9, [("copy", rows, code, True), ("rle", 2, 0, True), null], ("rle", 0, None, False), b"\x07\x01")
        # a COPY packet that holds uniform rows, of every group remainder
        for k in (1, 4, 6, 13):
            rows = T.literal_rows(k, 3, rng) + [b"\x02" * 16]
            shapes[f"uniform_rows_in_copy_code{code}_{k + 1}"] = (k + 1, [("copy", rows, code, False)], ("rle", 0, None, False), b"")
    # 4-byte RLE headers with counts below 128; RLE counts larger than rank + 1; null COPYs in front of an RLE that continues the same rank
    lit = T.literal_rows(3, 200, rng)
    shapes["long_rle_headers"] = (30, [("copy", lit, 0, False), ("rle", 10, 2, True), null, ("rle", 7, 2, False), ("copy", [], 3, False), ("rle", 5, 1, True), ("copy", [], 0, True),
                                       ("rle", 5, 0, False), null], ("rle", 0, None, False), b"\x09")
    shapes["rle_counts_above_rank_plus_one"] = (300, [("copy", [], 3, False), ("rle", 100, 3, False), null, ("rle", 130, 1, True), null, ("rle", 70, 200, False), null],
                                                ("rle", 0, None, False), b"")
    out = {}
    for name, (rows, packets, end, tail) in shapes.items():
        if middle:
            pad, tail = -rows % 8, b""
            if pad:
                packets, rows = packets + [("rle", pad, 77, False), null], rows + pad
        out[name] = (16 * rows + len(tail), T.write_stream(16 * rows + len(tail), packets + [end], tail))
    return out


GRAMMAR, GRAMMAR_MIDDLE = grammar_streams(False), grammar_streams(True)


def three_blocks(n, stream):
    """(container, bytes of blocks 0 and 2): `stream` as the middle block of three blocks of n bytes."""
    sides = varied(2 * n, n)
    a, b = sides[:n], sides[n:]
    return B.from_streams([B.block_stream(a), stream, B.block_stream(b)], 3 * n, n), a, b


@pytest.mark.parametrize("name", list(GRAMMAR))
def test_grammar_written_streams_as_one_block_containers_and_as_middle_blocks(hs, name):
    n, stream = GRAMMAR[name]
    want = T.model_decompress(stream)
    assert want is not None and len(want) == n
    assert check_decode(hs, name, B.from_streams([stream], n, (n + 127) // 128 * 128)) == (DONE, want)
    n, stream = GRAMMAR_MIDDLE[name]
    want = T.model_decompress(stream)
    assert want is not None and len(want) == n and n % 128 == 0
    c, a, b = three_blocks(n, stream)
    assert check_decode(hs, f"{name}: middle", c) == (DONE, a + want + b)


# ---- malformed ----

def malformed_streams(R):
    """The shapes of test_gpu_rle8_mmtf.py for a block of R rows (and no tail): (a good stream, name -> stream)."""
    rng = random.Random(33)
    rows = T.literal_rows(R + 1, 200, rng)
    more, rows = rows, rows[:R]
    n = 16 * R
    end, null = ("rle", 0, None, False), ("copy", [], 0, False)
    good = T.write_stream(n, [("copy", rows, 0, False), end])
    other = T.write_stream(n - 16, [("copy", rows[:-1], 0, False), end])
    return good, {
        "body_past_stream_size": T.write_stream(n, [("copy", rows, 0, False), end], stream_size=8 + 1 + 50),
        "long_body_past_stream_size": struct.pack("<III", n, 8 + 4 + n + 1, 0x1FFFFFF << 3 | 1) + b"".join(rows) + b"\x00",
        "copy_rows_past_R": T.write_stream(n, [("copy", more, 0, False), end]),
        "rle_rows_past_R": T.write_stream(n, [("copy", rows[:3], 0, False), ("rle", R - 2, 1, False), null, end]),
        "huge_rle_count": T.write_stream(n, [null, ("rle", 0x7FFFFFFF, 1, True), null, end]),
        "missing_terminator": T.write_stream(n, [("copy", rows, 0, False)]),
        "chain_goes_on_behind_the_rows": T.write_stream(n, [("copy", rows, 0, False), ("rle", 1, 0, False), null, end]),
        "rows_left_over": T.write_stream(n, [("copy", rows[:-1], 0, False), end]),
        "header_size_is_not_the_output_size": other,
        "stream_size_above_the_buffer": good[:4] + struct.pack("<I", len(good) + 1) + good[8:],
    }


def test_malformed_streams_as_one_block_containers(hs):
    good, bad = malformed_streams(6)
    bad = dict(bad, tail_past_stream_size=None)
    assert check_decode(hs, "good", B.from_streams([good], 96, 128)) == (DONE, T.model_decompress(good))
    for name, stream in bad.items():
        n = 96
        if name == "tail_past_stream_size":                                 # (only a last block has a tail: this shape has no middle-block form)
            n, stream = 99, T.write_stream(99, [("copy", T.literal_rows(6, 200, random.Random(2)), 0, False), ("rle", 0, None, False)], b"\x01\x02")
        c = B.from_streams([stream], n, 128)
        assert expected_blocks(c)[0] == MALFORMED, name
        status, out, clean = decompress_dev(hs, c)
        assert status == MALFORMED, name
        assert clean and out == b"\xEE" * n, f"{name}: the output or the canary around it was touched"
        assert hs.rle8_mmtf128_blocks_decompress_host(c, n + 64) == (ERR_FORMAT, b""), name


def test_malformed_streams_as_the_middle_block_of_three(hs):
    good, bad = malformed_streams(8)
    c, a, b = three_blocks(128, good)
    assert check_decode(hs, "good", c) == (DONE, a + T.model_decompress(good) + b)
    for name, stream in bad.items():
        c, a, b = three_blocks(128, stream)
        status, out = check_decode(hs, name, c)
        assert status == MALFORMED, name
        assert out == a + b"\xEE" * 128 + b, f"{name}: the block's range stays untouched, its neighbours are exact"


def test_a_cut_middle_stream_leaves_its_neighbours_whole(hs):
    data = varied(3 * 1152, 5)
    _, streams = B.split(B.build(data, 1152))
    c = B.from_streams([streams[0], streams[1][:-1], streams[2]], len(data), 1152)           # (the table is consistent: the stream is a byte short)
    status, out = check_decode(hs, "cut middle stream", c)
    assert status == MALFORMED
    assert out == data[:1152] + b"\xEE" * 1152 + data[2304:]


def test_bad_table_entries(hs):
    data = varied(3 * 128 + 17, 6)
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
    data8, data65 = varied(8 * 128 - 3, 7), varied(65 * 128 - 9, 8)
    n, stream = GRAMMAR_MIDDLE["long_rle_headers"]
    assert n == 512
    middle = T.model_decompress(stream)
    big = varied(5 * 512 - 11, 9)
    _, s5 = B.split(B.build(big, 512))
    hand = B.from_streams(s5[:2] + [stream] + s5[3:], len(big), 512)
    cut = B.from_streams(s5[:3] + [s5[3][:-1]] + s5[4:], len(big), 512)

    def hand_and_cut(name):
        assert check_decode(tuned, f"{name}: hand-made", hand) == (DONE, big[:1024] + middle + big[1536:])
        status, out = check_decode(tuned, f"{name}: cut", cut)
        assert status == MALFORMED and out == big[:1536] + b"\xEE" * 512 + big[2048:]

    for in_flight, blocks_data in ((1, data8), (3, data8), (0, data8), (64, data65), (0, data65)):
        tuned.rle8_mmtf128_blocks_tuning(in_flight)
        want = check_encode(tuned, f"in flight {in_flight}", blocks_data, 128)
        assert check_decode(tuned, f"in flight {in_flight}", want) == (DONE, blocks_data)
        hand_and_cut(f"in flight {in_flight}")
    tuned.rle8_mmtf128_blocks_tuning(3)
    wide = varied(3 * 4096 + 17, 10)
    for span in (1, 7, 63, 0):
        tuned.rle8_mmtf_tuning(span)
        for bs, d in ((128, data8), (1152, placed(1152, shapes(1152)["3bit_group_across_row_64"], 5)), (4096, wide)):
            want = check_encode(tuned, f"span rows {span} / {bs}", d, bs)
            assert check_decode(tuned, f"span rows {span} / {bs}", want) == (DONE, d)
        hand_and_cut(f"span rows {span}")


# ---- graph ----

def test_graph_capture_and_replay(tuned):
    """Compress then decompress (a linear chain) captured once on a side stream, two groups each, and replayed on new bytes with the workspaces
    refilled with garbage.  (The container's sizes are part of the captured decode call: the replays' inputs give containers of the same size.)"""
    import torch

    tuned.rle8_mmtf128_blocks_tuning(3)
    bs = 128
    inputs = [B.data_from_block_specs([[("copy", 3, 3), ("rle", 5, r)]] * 5 + [[("copy", 2, 200), ("rle", 1, r + 1)]], bs, tail=bytes([r, 1, 2, 3, 4]), seed=r) for r in (1, 2, 3)]
    n = len(inputs[0])
    assert n == 5 * 128 + 48 + 5
    wants = [B.build(d, bs) for d in inputs]
    assert len({len(c) for c in wants}) == 1 and len(set(wants)) == 3
    total, cap = len(wants[0]), tuned.rle8_mmtf128_blocks_bound(n, bs)
    info = info_of(tuned, wants[0])
    src = to_dev(inputs[0])
    enc = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dec = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    ws1 = torch.full((tuned.rle8_mmtf128_blocks_workspace_size(0, n, bs),), 0xC3, dtype=torch.uint8, device="cuda")
    ws2 = torch.full((tuned.rle8_mmtf128_blocks_workspace_size(1, n, bs),), 0xC3, dtype=torch.uint8, device="cuda")
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    words = torch.full((2,), -1, dtype=torch.int32, device="cuda")

    def both(stream):
        tuned.rle8_mmtf128_blocks_compress_dev(src, enc[:cap], size, words[0:1], ws1, block_size=bs, stream=stream)
        tuned.rle8_mmtf128_blocks_decompress_dev(enc[:total], info, dec[:n], words[1:2], ws2, stream=stream)

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
