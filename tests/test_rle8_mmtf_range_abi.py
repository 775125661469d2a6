"""The exports of the rle8_mmtf128 checkpoints and byte-range decode without a GPU (include/hsrle.h section 5): the names, hsrle_rle8_mmtf128_checkpoints_bound,
the header validation of hsrle_rle8_mmtf128_checkpoints_info_host on hand-built headers, hsrle_rle8_mmtf128_range_workspace_size, and every return value of
the device entries that is decided on the host."""
import ctypes
import os
import struct

import pytest

import hsrle
import rle8_mmtf_index_testlib as X
import rle8_mmtf_range_testlib as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "hypersonic-rle-kit_amd", "libhsrle_hip.so")
NAMES = ["hsrle_rle8_mmtf128_checkpoints_bound", "hsrle_rle8_mmtf128_checkpoints_info_host", "hsrle_rle8_mmtf128_checkpoints_build_dev_async",
         "hsrle_rle8_mmtf128_range_workspace_size", "hsrle_rle8_mmtf128_decompress_range_dev_async", "hsrle_rle8_mmtf128_checkpoints_build_host",
         "hsrle_rle8_mmtf128_decompress_range_host"]
OK, ERR_ARGUMENT, ERR_CAPACITY, ERR_FORMAT = 0, 1, 2, 3
MAX_IN = 1 << 30


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess

        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(REPO, "hypersonic-rle-kit_amd")])
    return hsrle.declare(ctypes.CDLL(LIB))


def test_names_are_exported_and_bound(lib):
    for nm in NAMES:
        assert hasattr(lib, nm) and nm in hsrle.SIGNATURES, nm
    assert hsrle.RLE8_MMTF_CHECKPOINT == 4 and hsrle.Rle8MmtfCheckpointsInfo is not hsrle.MonoIndexInfo
    assert ctypes.sizeof(hsrle.Rle8MmtfCheckpointsInfo) == 32


def test_checkpoints_bound(lib):
    B = lib.hsrle_rle8_mmtf128_checkpoints_bound
    for rows in (1, 63, 65, 96, (1 << 24) + 64, 1 << 25):
        assert B(16 * 4096, rows) == 0, rows
    assert B(MAX_IN + 1, 64) == 0 and B(MAX_IN + 1, 0) == 0
    for ck in (64, 128, 1 << 24):
        for rows, count in ((0, 0), (1, 0), (ck, 0), (ck + 1, 1), (2 * ck, 1), (2 * ck + 1, 2)):
            if 16 * rows + 15 <= MAX_IN:
                assert B(16 * rows, ck) == B(16 * rows + 15, ck) == 64 + 4096 * count, (ck, rows)
    assert B(15, 64) == 64
    assert B(MAX_IN, 0) == B(MAX_IN, 65536) == 64 + 4096 * 1023            # the default: 1 MiB of output per checkpoint
    assert B(MAX_IN, 64) == 64 + 4096 * ((1 << 20) - 1)
    for name, data in X.encoder_inputs().items():                          # the bound is exact: the model's sidecar has this size
        for ck in G.CHECKPOINT_ROWS:
            assert len(G.model_checkpoints(data, ck, 10)) == B(len(data), ck), name


def header(magic=G.MAGIC, version=1, header_bytes=64, in_size=16 * 1000, stream_size=500, rows=64, count=15, size=None, pad=bytes(24)):
    return magic + struct.pack("<IIIIIIQ", version, header_bytes, in_size, stream_size, rows, count, 64 + 4096 * count if size is None else size) + pad


def test_checkpoints_info_host(lib):
    F = lib.hsrle_rle8_mmtf128_checkpoints_info_host
    info = hsrle.Rle8MmtfCheckpointsInfo()
    good = header() + bytes(15 * 4096)
    assert F(good, len(good), ctypes.byref(info)) == OK
    assert (info.version, info.headerBytes, info.uncompressedSize, info.streamSize, info.checkpointRows, info.checkpointCount, info.size) == (1, 64, 16000, 500, 64, 15, 64 + 15 * 4096)
    assert F(good + bytes(9), len(good) + 9, ctypes.byref(info)) == OK                       # a buffer larger than the sidecar
    assert F(header(in_size=16 * 64 + 5, count=0), 64, ctypes.byref(info)) == OK and info.checkpointCount == 0
    assert F(header(in_size=13, count=0), 64, ctypes.byref(info)) == OK
    assert F(header(rows=1 << 24, count=0), 64, ctypes.byref(info)) == OK and info.checkpointRows == 1 << 24
    bad = {
        "magic": header(magic=b"HSRLEMFD"), "the_index_magic": header(magic=X.MAGIC), "the_rle8_sh_container_magic": header(magic=b"HSRLESHB"),
        "the_rle8_mmtf128_container_magic": header(magic=b"HSRLEMFB"), "version": header(version=2), "header_bytes": header(header_bytes=80), "no_size": header(in_size=0, count=0),
        "size_above_2^30": header(in_size=MAX_IN + 1), "stream_size": header(stream_size=9), "rows_0": header(rows=0), "rows_odd": header(rows=96), "rows_large": header(rows=1 << 25),
        "one_checkpoint_more": header(count=16), "one_checkpoint_fewer": header(count=14), "sidecar_size": header(size=64 + 4096 * 15 + 16),
        "sidecar_size_high_word": header(size=(1 << 32) + 64 + 4096 * 15), "not_zero_behind": header(pad=bytes(23) + b"\x01"),
    }
    for name, h in bad.items():
        buf = h + bytes(17 * 4096)
        assert F(buf, len(buf), ctypes.byref(info)) == ERR_FORMAT, name
    assert F(good, len(good) - 1, ctypes.byref(info)) == ERR_FORMAT                          # the buffer ends inside the checkpoints
    assert F(good, 63, ctypes.byref(info)) == ERR_FORMAT
    assert F(None, 64, ctypes.byref(info)) == ERR_ARGUMENT and F(good, len(good), None) == ERR_ARGUMENT
    assert hsrle.rle8_mmtf128_checkpoints_info(good).checkpointCount == 15
    with pytest.raises(hsrle.HsrleError):
        hsrle.rle8_mmtf128_checkpoints_info(bad["magic"])


def test_the_other_info_functions_refuse_the_checkpoint_magic(lib):
    side = header() + bytes(15 * 4096)
    idx, blk = hsrle.Rle8MmtfIndexInfo(), hsrle.Rle8ShBlocksInfo()
    assert lib.hsrle_rle8_mmtf128_index_info_host(side, len(side), ctypes.byref(idx)) == ERR_FORMAT
    assert lib.hsrle_rle8_mmtf128_blocks_info_host(side, len(side), ctypes.byref(blk)) == ERR_FORMAT
    assert lib.hsrle_rle8_sh_blocks_info_host(side, len(side), ctypes.byref(blk)) == ERR_FORMAT


def test_range_workspace_size(lib):
    W = lib.hsrle_rle8_mmtf128_range_workspace_size
    assert W(0, 64, 64) == 0 and W(MAX_IN + 1, 64, 64) == 0
    for spacing, ck in ((96, 64), (64, 96), (1 << 21, 64), (64, 1 << 25), (32, 64), (64, 32)):
        assert W(4096, spacing, ck) == 0, (spacing, ck)
    assert W(4096, 0, 0) != 0 and W(4096, 0, 0) in [W(4096, spacing, 65536) for spacing in (256, 1024, 4096)]      # the two defaults
    # three arguments, none of them the stream's size: monotone in the length, for every spacing pair
    for spacing, ck in ((64, 64), (64, 128), (1024, 65536), (4096, 16384)):
        sizes = [W(length, spacing, ck) for length in (1, 15, 16, 17, 1024, 4096, 65536, 1 << 20, (1 << 20) + 1, 16 << 20, MAX_IN)]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (spacing, ck)
        assert sizes[-2] > sizes[0]
    # a range decode of 1 MiB needs far less than the whole decode of a large stream, and a whole small stream's range fits its bound
    assert W(1 << 20, 1024, 65536) < lib.hsrle_rle8_mmtf128_workspace_size(1, 64 << 20) // 8


def test_dev_async_argument_checks(lib):
    # host buffers stand in for device pointers: every call below is refused on the host, before anything could touch them
    src, dst, idx, side, ws, words = (ctypes.create_string_buffer(n) for n in (4096, 4096, 4096, 8192, 64, 32))
    a, b, x, c, w = (ctypes.addressof(t) for t in (src, dst, idx, side, ws))
    s = (ctypes.addressof(words) + 7) & ~7
    z = s + 8
    big = 1 << 40
    n = 16 * 100 + 3
    info = hsrle.Rle8MmtfIndexInfo()
    index = struct.pack("<8sIIIIIIQ", X.MAGIC, 1, 64, n, 100, 64, 1, 80) + bytes(24 + 16)
    assert lib.hsrle_rle8_mmtf128_index_info_host(index, len(index), ctypes.byref(info)) == OK
    ck = hsrle.Rle8MmtfCheckpointsInfo()
    good = header(in_size=n, stream_size=100, count=1) + bytes(4096)
    assert lib.hsrle_rle8_mmtf128_checkpoints_info_host(good, len(good), ctypes.byref(ck)) == OK
    I, K = ctypes.byref(info), ctypes.byref(ck)

    B = lib.hsrle_rle8_mmtf128_checkpoints_build_dev_async
    cap = lib.hsrle_rle8_mmtf128_checkpoints_bound(n, 64)
    need = lib.hsrle_rle8_mmtf128_workspace_size(1, n)
    assert cap == 64 + 4096
    assert B(a, 100, x, I, 64, c, cap, z, s, w, need - 1, None) == ERR_CAPACITY              # (a short workspace: the last check, nothing is enqueued)
    assert B(a, 100, x, I, 64, c, cap - 1, z, s, w, big, None) == ERR_CAPACITY
    assert B(None, 100, x, I, 64, c, cap, z, s, w, big, None) == ERR_ARGUMENT
    assert B(a, 0, x, I, 64, c, cap, z, s, w, big, None) == ERR_ARGUMENT
    assert B(a, 100, None, I, 64, c, cap, z, s, w, big, None) == ERR_ARGUMENT
    assert B(a, 100, x, None, 64, c, cap, z, s, w, big, None) == ERR_ARGUMENT
    assert B(a, 100, x, I, 96, c, cap, z, s, w, big, None) == ERR_ARGUMENT
    assert B(a, 100, x, I, 64, None, cap, z, s, w, big, None) == ERR_ARGUMENT
    assert B(a, 100, x, I, 64, c, cap, None, s, w, big, None) == ERR_ARGUMENT
    assert B(a, 100, x, I, 64, c, cap, z + 4, s, w, big, None) == ERR_ARGUMENT               # the size word is 8 bytes
    assert B(a, 100, x, I, 64, c, cap, z, None, w, big, None) == ERR_ARGUMENT
    assert B(a, 100, x, I, 64, c, cap, z, s + 2, w, big, None) == ERR_ARGUMENT
    assert B(a, 100, x, I, 64, c, cap, z, s, None, big, None) == ERR_ARGUMENT
    assert B(a, 100, x, I, 64, a + 50, cap, z, s, w, big, None) == ERR_ARGUMENT              # checkpoints over the stream
    assert B(a, 100, x, I, 64, x + 50, cap, z, s, w, big, None) == ERR_ARGUMENT              # ... over the index
    t = hsrle.Rle8MmtfIndexInfo.from_buffer_copy(info)
    t.recordBytes = 96
    assert B(a, 100, x, ctypes.byref(t), 64, c, cap, z, s, w, big, None) == ERR_ARGUMENT

    D = lib.hsrle_rle8_mmtf128_decompress_range_dev_async
    need = lib.hsrle_rle8_mmtf128_range_workspace_size(200, 64, 64)
    assert 0 < need
    assert D(a, 100, x, I, c, K, 16, 200, b, 200, s, w, 63, None) == ERR_CAPACITY             # (a short workspace: the last check, nothing is enqueued)
    assert D(a, 100, x, I, c, K, 16, 0, b, 0, s, w, 0, None) == OK                            # length 0: nothing to do
    assert D(a, 100, x, I, c, K, n, 0, b, 0, s, w, 0, None) == OK
    assert D(None, 100, x, I, c, K, 16, 200, b, 200, s, w, big, None) == ERR_ARGUMENT
    assert D(a, 0, x, I, c, K, 16, 200, b, 200, s, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, None, I, c, K, 16, 200, b, 200, s, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, x, None, c, K, 16, 200, b, 200, s, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, x, I, None, K, 16, 200, b, 200, s, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, x, I, c, None, 16, 200, b, 200, s, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, x, I, c, K, 16, 200, None, 200, s, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, x, I, c, K, 16, 200, b, 200, None, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, x, I, c, K, 16, 200, b, 200, s + 2, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, x, I, c, K, 16, 200, b, 200, s, None, big, None) == ERR_ARGUMENT
    assert D(a, 100, x, I, c, K, n - 199, 200, b, 200, s, w, big, None) == ERR_ARGUMENT       # offset + length > uncompressedSize
    assert D(a, 100, x, I, c, K, n + 1, 0, b, 0, s, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, x, I, c, K, 1 << 63, 1 << 63, b, 200, s, w, big, None) == ERR_ARGUMENT   # (a sum that wraps)
    assert D(a, 100, x, I, c, K, 16, 200, b, 199, s, w, big, None) == ERR_ARGUMENT            # outCapacity < length
    assert D(a, 100, x, I, c, K, 16, 200, a + 50, 200, s, w, big, None) == ERR_ARGUMENT       # output over the stream
    assert D(a, 100, x, I, c, K, 16, 200, c + 4000, 200, s, w, big, None) == ERR_ARGUMENT     # ... over the checkpoints
    for field, value in (("uncompressedSize", n + 16), ("streamSize", 101)):                  # two infos that disagree
        t = hsrle.Rle8MmtfCheckpointsInfo.from_buffer_copy(ck)
        setattr(t, field, value)
        assert D(a, 100, x, I, c, ctypes.byref(t), 16, 200, b, 200, s, w, big, None) == ERR_ARGUMENT, field
    for field, value in (("version", 2), ("headerBytes", 0), ("checkpointRows", 96), ("checkpointCount", 2), ("size", 64)):
        t = hsrle.Rle8MmtfCheckpointsInfo.from_buffer_copy(ck)
        setattr(t, field, value)
        assert D(a, 100, x, I, c, ctypes.byref(t), 16, 200, b, 200, s, w, big, None) == ERR_ARGUMENT, field
    assert dst.raw == bytes(4096) and side.raw == bytes(8192) and words.raw == bytes(32)

    # the host-pointer calls: what is decided before a device is touched
    size = ctypes.c_uint64(7)
    H, R = lib.hsrle_rle8_mmtf128_checkpoints_build_host, lib.hsrle_rle8_mmtf128_decompress_range_host
    stream = struct.pack("<II", n, 100) + bytes(92)
    assert H(None, 100, index, len(index), 64, c, cap, ctypes.byref(size)) == ERR_ARGUMENT and H(stream, 100, None, len(index), 64, c, cap, ctypes.byref(size)) == ERR_ARGUMENT
    assert H(stream, 100, index, len(index), 64, None, cap, ctypes.byref(size)) == ERR_ARGUMENT and H(stream, 100, index, len(index), 64, c, cap, None) == ERR_ARGUMENT
    assert H(stream, 7, index, len(index), 64, c, cap, ctypes.byref(size)) == ERR_ARGUMENT and H(stream, 100, index, len(index), 33, c, cap, ctypes.byref(size)) == ERR_ARGUMENT
    assert H(stream, 100, index, len(index) - 1, 64, c, cap, ctypes.byref(size)) == ERR_FORMAT
    assert H(stream, 100, good, len(good), 64, c, cap, ctypes.byref(size)) == ERR_FORMAT      # the checkpoints where the index belongs
    assert H(stream, 100, index, len(index), 64, c, cap - 1, ctypes.byref(size)) == ERR_CAPACITY
    assert R(None, 100, index, len(index), good, len(good), 16, 200, b, 200) == ERR_ARGUMENT and R(stream, 100, None, len(index), good, len(good), 16, 200, b, 200) == ERR_ARGUMENT
    assert R(stream, 100, index, len(index), None, len(good), 16, 200, b, 200) == ERR_ARGUMENT and R(stream, 100, index, len(index), good, len(good), 16, 200, None, 200) == ERR_ARGUMENT
    assert R(stream, 100, index, len(index) - 1, good, len(good), 16, 200, b, 200) == ERR_FORMAT
    assert R(stream, 100, index, len(index), good, len(good) - 1, 16, 200, b, 200) == ERR_FORMAT
    assert R(stream, 100, index, len(index), index, len(index), 16, 200, b, 200) == ERR_FORMAT          # the index where the checkpoints belong
    assert R(stream, 100, index, len(index), good, len(good), n - 199, 200, b, 200) == ERR_ARGUMENT
    assert R(stream, 100, index, len(index), good, len(good), 16, 200, b, 199) == ERR_ARGUMENT
    assert R(stream, 100, index, len(index), good, len(good), 16, 0, b, 0) == OK
    assert size.value == 7 and dst.raw == bytes(4096)
