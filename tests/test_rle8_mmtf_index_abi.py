"""The exports of the rle8_mmtf128 entry index without a GPU (include/hsrle.h section 5): the names, hsrle_rle8_mmtf128_index_bound, the header
validation of hsrle_rle8_mmtf128_index_info_host on hand-built headers, and every return value of the device entries that is decided on the host."""
import ctypes
import os
import struct

import pytest

import hsrle
import rle8_mmtf_index_testlib as X

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "hypersonic-rle-kit_amd", "libhsrle_hip.so")
NAMES = ["hsrle_rle8_mmtf128_index_bound", "hsrle_rle8_mmtf128_index_info_host", "hsrle_rle8_mmtf128_compress_indexed_dev_async", "hsrle_rle8_mmtf128_index_build_dev_async",
         "hsrle_rle8_mmtf128_decompress_indexed_dev_async", "hsrle_rle8_mmtf128_index_build_host", "hsrle_rle8_mmtf128_decompress_indexed_host"]
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
    assert hsrle.RLE8_MMTF_INDEX == 3 and hsrle.Rle8MmtfIndexInfo is hsrle.MonoIndexInfo


def test_index_bound(lib):
    B = lib.hsrle_rle8_mmtf128_index_bound
    for spacing in (1, 63, 65, 96, (1 << 20) + 64, 1 << 21):
        assert B(4096, spacing) == 0, spacing
    assert B(MAX_IN + 1, 64) == 0 and B(MAX_IN + 1, 0) == 0
    # windows 1 .. that hold a row: an entry each at the most
    for size, spacing, entries in ((0, 64, 0), (15, 64, 0), (16 * 64, 64, 0), (16 * 64 + 15, 64, 0), (16 * 65, 64, 1), (16 * 128, 64, 1), (16 * 129, 64, 2), (16 * 129, 128, 1),
                                   (MAX_IN, 64, (1 << 20) - 1), (MAX_IN, 1 << 20, 63)):
        assert B(size, spacing) == 64 + 16 * entries, (size, spacing)
    assert B(MAX_IN, 0) in (B(MAX_IN, 256), B(MAX_IN, 1024), B(MAX_IN, 4096))               # the default is one of the measured spacings
    # the model's index of every case fits
    import rle8_mmtf_testlib as T

    for name, data in X.encoder_inputs().items():
        for spacing in X.SPACINGS:
            assert len(X.model_index(T.model_compress(data), spacing)) <= B(len(data), spacing), name


def header(magic=X.MAGIC, version=1, header_bytes=64, in_size=16 * 1000, stream_size=500, spacing=64, count=3, size=None, pad=bytes(24)):
    return magic + struct.pack("<IIIIIIQ", version, header_bytes, in_size, stream_size, spacing, count, 64 + 16 * count if size is None else size) + pad


def test_index_info_host(lib):
    F = lib.hsrle_rle8_mmtf128_index_info_host
    info = hsrle.Rle8MmtfIndexInfo()
    good = header() + bytes(48)
    assert F(good, len(good), ctypes.byref(info)) == OK
    assert (info.version, info.codec, info.uncompressedSize, info.compressedSize, info.spacing, info.recordCount, info.recordBytes, info.indexBytes) == (
        1, hsrle.RLE8_MMTF_INDEX_CODEC, 16000, 500, 64, 3, 16, 112)
    assert bytes(info.streamHead) == bytes(16)
    assert F(good + bytes(9), len(good) + 9, ctypes.byref(info)) == OK                      # a buffer larger than the index
    assert F(header(count=0), 64, ctypes.byref(info)) == OK and info.recordCount == 0
    assert F(header(in_size=16 * 1000, count=15) + bytes(240), 64 + 240, ctypes.byref(info)) == OK          # (1000 - 1) // 64 entries at the most
    bad = {
        "magic": header(magic=b"HSRLEMFJ"), "version": header(version=2), "header_bytes": header(header_bytes=80), "no_size": header(in_size=0), "size_above_2^30": header(in_size=MAX_IN + 1),
        "stream_size": header(stream_size=9), "spacing_0": header(spacing=0), "spacing_odd": header(spacing=96), "spacing_large": header(spacing=1 << 21),
        "too_many_entries": header(count=16, in_size=16 * 1000), "index_size": header(size=64 + 16 * 3 + 16), "index_size_high_word": header(size=(1 << 32) + 112),
        "not_zero_behind": header(pad=bytes(23) + b"\x01"),
    }
    for name, h in bad.items():
        buf = h + bytes(512)
        assert F(buf, len(buf), ctypes.byref(info)) == ERR_FORMAT, name
    assert F(good, len(good) - 1, ctypes.byref(info)) == ERR_FORMAT                          # the buffer ends inside the entries
    assert F(good, 63, ctypes.byref(info)) == ERR_FORMAT
    assert F(None, 64, ctypes.byref(info)) == ERR_ARGUMENT and F(good, len(good), None) == ERR_ARGUMENT
    assert hsrle.rle8_mmtf128_index_info(good).recordCount == 3
    with pytest.raises(hsrle.HsrleError):
        hsrle.rle8_mmtf128_index_info(bad["magic"])


def test_dev_async_argument_checks(lib):
    # host buffers stand in for device pointers: every call below is refused on the host, before anything could touch them
    src, dst, idx, ws, words = (ctypes.create_string_buffer(n) for n in (4096, 4096, 4096, 64, 32))
    a, b, x, w = (ctypes.addressof(t) for t in (src, dst, idx, ws))
    s = (ctypes.addressof(words) + 7) & ~7
    z = s + 8
    big = 1 << 40
    C, B, D = lib.hsrle_rle8_mmtf128_compress_indexed_dev_async, lib.hsrle_rle8_mmtf128_index_build_dev_async, lib.hsrle_rle8_mmtf128_decompress_indexed_dev_async
    need = lib.hsrle_rle8_mmtf128_workspace_size(0, 2048)
    cap = lib.hsrle_rle8_mmtf128_index_bound(2048, 64)
    assert cap == 64 + 16
    assert C(None, 2048, b, 4096, s, s + 4, w, big, 64, x, cap, z, None) == ERR_ARGUMENT
    assert C(a, 2048, b, 4096, s, s + 4, w, big, 64, None, cap, z, None) == ERR_ARGUMENT
    assert C(a, 2048, b, 4096, s, s + 4, w, big, 64, x, cap, None, None) == ERR_ARGUMENT
    assert C(a, 2048, b, 4096, s, s + 4, w, big, 64, x, cap, z + 4, None) == ERR_ARGUMENT      # the index size word is 8 bytes
    assert C(a, 2048, b, 4096, s, s + 4, w, big, 100, x, cap, z, None) == ERR_ARGUMENT         # spacing
    assert C(a, 2048, b, 4096, s, s + 4, w, big, 64, a + 100, cap, z, None) == ERR_ARGUMENT    # index over the input
    assert C(a, 2048, b, 4096, s, s + 4, w, big, 64, b + 4000, cap, z, None) == ERR_ARGUMENT   # index over the output
    assert C(a, 0, b, 4096, s, s + 4, w, big, 64, x, cap, z, None) == ERR_ARGUMENT
    assert C(a, 2048, b, 4096, s, s + 4, w, big, 64, x, cap - 1, z, None) == ERR_CAPACITY
    assert C(a, 2048, b, 2048 + 7, s, s + 4, w, big, 64, x, cap, z, None) == ERR_CAPACITY
    assert C(a, 2048, b, 4096, s, s + 4, w, need - 1, 64, x, cap, z, None) == ERR_CAPACITY
    assert B(None, 100, 2048, 64, x, cap, z, s, None) == ERR_ARGUMENT
    assert B(a, 100, 2048, 64, None, cap, z, s, None) == ERR_ARGUMENT
    assert B(a, 100, 2048, 64, x, cap, None, s, None) == ERR_ARGUMENT
    assert B(a, 100, 2048, 64, x, cap, z, None, None) == ERR_ARGUMENT
    assert B(a, 0, 2048, 64, x, cap, z, s, None) == ERR_ARGUMENT
    assert B(a, 100, 0, 64, x, cap, z, s, None) == ERR_ARGUMENT
    assert B(a, 100, MAX_IN + 1, 64, x, big, z, s, None) == ERR_ARGUMENT
    assert B(a, 100, 2048, 32, x, cap, z, s, None) == ERR_ARGUMENT
    assert B(a, 100, 2048, 64, x, cap, z + 4, s, None) == ERR_ARGUMENT
    assert B(a, 100, 2048, 64, x, cap, z, s + 2, None) == ERR_ARGUMENT
    assert B(a, 100, 2048, 64, a + 50, cap, z, s, None) == ERR_ARGUMENT                        # index over the stream
    assert B(a, 100, 2048, 64, x, cap - 1, z, s, None) == ERR_CAPACITY
    info = hsrle.Rle8MmtfIndexInfo()
    assert lib.hsrle_rle8_mmtf128_index_info_host(header(in_size=2048, stream_size=100, count=1) + bytes(16), 80, ctypes.byref(info)) == OK
    need = lib.hsrle_rle8_mmtf128_workspace_size(1, 2048)
    ok = lambda i: D(a, 100, x, ctypes.byref(i), b, 2048, s, w, need - 1, None)               # (a short workspace: the last check, nothing is enqueued)
    assert ok(info) == ERR_CAPACITY
    assert D(None, 100, x, ctypes.byref(info), b, 2048, s, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, None, ctypes.byref(info), b, 2048, s, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, x, None, b, 2048, s, w, big, None) == ERR_ARGUMENT
    assert D(a, 100, x, ctypes.byref(info), b, 2064, s, w, big, None) == ERR_ARGUMENT          # the index is of another size
    assert D(a, 100, b + 2000, ctypes.byref(info), b, 2048, s, w, big, None) == ERR_ARGUMENT   # index over the output
    for field, value in (("version", 2), ("codec", 0), ("recordBytes", 96), ("spacing", 96), ("recordCount", 2)):
        t = hsrle.Rle8MmtfIndexInfo.from_buffer_copy(info)
        setattr(t, field, value)
        assert ok(t) == ERR_ARGUMENT, field
    assert dst.raw == bytes(4096) and idx.raw == bytes(4096)
    # the host-pointer calls: what is decided before a device is touched
    size = ctypes.c_uint64(7)
    H, G = lib.hsrle_rle8_mmtf128_index_build_host, lib.hsrle_rle8_mmtf128_decompress_indexed_host
    stream = struct.pack("<II", 2048, 100) + bytes(92)
    assert H(None, 100, 64, x, cap, ctypes.byref(size)) == ERR_ARGUMENT and H(stream, 100, 64, None, cap, ctypes.byref(size)) == ERR_ARGUMENT
    assert H(stream, 7, 64, x, cap, ctypes.byref(size)) == ERR_ARGUMENT and H(stream, 100, 33, x, cap, ctypes.byref(size)) == ERR_ARGUMENT
    assert H(stream, 100, 64, x, cap - 1, ctypes.byref(size)) == ERR_CAPACITY
    assert H(struct.pack("<II", 0, 100) + bytes(92), 100, 64, x, cap, ctypes.byref(size)) == ERR_FORMAT
    index = header(in_size=2048, stream_size=100, count=1) + bytes(16)
    assert G(None, 100, index, 80, b, 4096, ctypes.byref(size)) == ERR_ARGUMENT and G(stream, 100, None, 80, b, 4096, ctypes.byref(size)) == ERR_ARGUMENT
    assert G(stream, 100, index, 79, b, 4096, ctypes.byref(size)) == ERR_FORMAT
    assert G(stream, 100, index, 80, b, 2047, ctypes.byref(size)) == ERR_CAPACITY
    assert size.value == 7 and dst.raw == bytes(4096)
