"""The rle8_mmtf128 block container's exports without a GPU (include/hsrle.h section 5): the names, the bound against the Python helper, a workspace that
depends on the blocks in flight and not on the input size, the header check of info_host field by field, the three container magics refused by the
other families' info functions, and every return value of the host calls and the two _dev_async calls that is decided on the host before a device is
touched, in the documented order."""
import ctypes
import os
import struct

import pytest

import hsrle

import rle8_mmtf_blocks_testlib as B
import rle8_mmtf_testlib as T
import rle8_sh_blocks_testlib as SHB

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "hypersonic-rle-kit_amd", "libhsrle_hip.so")

NAMES = ["hsrle_rle8_mmtf128_blocks_bound", "hsrle_rle8_mmtf128_blocks_workspace_size", "hsrle_rle8_mmtf128_blocks_info_host", "hsrle_rle8_mmtf128_blocks_info_dev",
         "hsrle_rle8_mmtf128_compress_blocks_dev_async", "hsrle_rle8_mmtf128_decompress_blocks_dev_async", "hsrle_rle8_mmtf128_compress_blocks_host",
         "hsrle_rle8_mmtf128_decompress_blocks_host", "hsrle_rle8_mmtf128_blocks_tuning"]
OK, ERR_ARGUMENT, ERR_CAPACITY, ERR_FORMAT = 0, 1, 2, 3
DEFAULT_IN_FLIGHT = {128: 8192, 1024: 8192, 4096: 8192, 16384: 2048, 65536: 512, 1 << 20: 256}     # 32 MiB a group, 256 .. 8192 blocks: the rle8_sh container's

Info, KitInfo = hsrle.Rle8ShBlocksInfo, hsrle.ContainerInfo


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess

        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(REPO, "hypersonic-rle-kit_amd")])
    L = hsrle.declare(ctypes.CDLL(LIB))
    L.hsrle_rle8_mmtf128_blocks_tuning(0)
    L.hsrle_rle8_mmtf_tuning(0)
    yield L
    L.hsrle_rle8_mmtf128_blocks_tuning(0)
    L.hsrle_rle8_mmtf_tuning(0)


def test_names_are_exported(lib):
    for nm in NAMES:
        assert hasattr(lib, nm), nm
        assert nm in hsrle.SIGNATURES, nm
    for nm in ("bound", "workspace_size", "tuning", "info", "compress_dev", "decompress_dev", "compress_host", "decompress_host"):
        assert callable(getattr(hsrle, "rle8_mmtf128_blocks_" + nm)), nm


def test_bound_is_the_helpers(lib):
    for bs in (128, 1152, 4096, 65536, 1 << 20):
        for n in (1, bs - 1, bs, bs + 1, 3 * bs + 17, 100 * bs, (1 << 30) + 5):
            assert lib.hsrle_rle8_mmtf128_blocks_bound(n, bs) == B.bound(n, bs), (n, bs)
    assert lib.hsrle_rle8_mmtf128_blocks_bound(10000, 0) == B.bound(10000, 4096)            # block size 0 means 4096
    # header + table + the blocks' own bytes + 13 each + pad, spelled out once
    assert lib.hsrle_rle8_mmtf128_blocks_bound(300, 128) == 64 + 8 * 4 + 2 * (128 + 13) + (44 + 13) + 32
    for bs in (1, 64, 127, 129, 192 + 1, (1 << 20) + 128, 1 << 21, 0xFFFFFF80):
        assert lib.hsrle_rle8_mmtf128_blocks_bound(4096, bs) == 0, bs
    assert lib.hsrle_rle8_mmtf128_blocks_bound(0, 4096) == 0 and lib.hsrle_rle8_mmtf128_blocks_bound(0, 0) == 0


def test_bound_counts_2_to_the_32_blocks_as_too_many(lib):
    assert lib.hsrle_rle8_mmtf128_blocks_bound(128 * ((1 << 32) - 1), 128) == B.bound(128 * ((1 << 32) - 1), 128) != 0
    assert lib.hsrle_rle8_mmtf128_blocks_bound(128 * ((1 << 32) - 1) + 1, 128) == 0 == B.bound(128 * ((1 << 32) - 1) + 1, 128)
    assert lib.hsrle_rle8_mmtf128_blocks_workspace_size(0, 128 * ((1 << 32) - 1) + 1, 128) == 0


def test_workspace_depends_on_the_blocks_in_flight_not_on_the_input(lib):
    try:
        for decode in (0, 1):
            for bs, fly in DEFAULT_IN_FLIGHT.items():
                lib.hsrle_rle8_mmtf128_blocks_tuning(0)
                W = lambda n: lib.hsrle_rle8_mmtf128_blocks_workspace_size(decode, n, bs)  # noqa: E731
                slot = W(1) - 512                                                           # 512 bytes of the call's own, then a slot per block in flight
                assert W(0) == 0
                assert slot >= bs + 16 + 256                                                # a slot holds the block's rank buffer and its control words
                assert slot <= 3 * bs + 1024                                                # ... and tables smaller than the block (16 bytes per row at most)
                assert W(1) == W(bs) == 512 + slot
                assert W(bs + 1) == 512 + 2 * slot
                assert W(fly * bs) == W(fly * bs + 1) == W(50 * fly * bs) == 512 + fly * slot, (decode, bs)
                assert W((fly - 1) * bs) == 512 + (fly - 1) * slot
                for tuned in (1, 3, 64):
                    lib.hsrle_rle8_mmtf128_blocks_tuning(tuned)
                    assert W(tuned * bs) == W(1000 * bs + 5) == 512 + tuned * slot
                    assert W(bs) == 512 + slot
        lib.hsrle_rle8_mmtf128_blocks_tuning(0)
        assert lib.hsrle_rle8_mmtf128_blocks_workspace_size(0, 1 << 20, 0) == lib.hsrle_rle8_mmtf128_blocks_workspace_size(0, 1 << 20, 4096)
        assert lib.hsrle_rle8_mmtf128_blocks_workspace_size(1, 1 << 30, 4096) < 1 << 27    # 8192 slots of 4 KiB blocks: under 128 MiB
        for bs in (64, 4097, 1 << 21):
            assert lib.hsrle_rle8_mmtf128_blocks_workspace_size(0, 1 << 20, bs) == 0 == lib.hsrle_rle8_mmtf128_blocks_workspace_size(1, 1 << 20, bs)
        # rows per span (hsrle_rle8_mmtf_tuning): more spans, a larger compress slot; the decode slot has no spans
        enc, dec = lib.hsrle_rle8_mmtf128_blocks_workspace_size(0, 4096, 4096), lib.hsrle_rle8_mmtf128_blocks_workspace_size(1, 4096, 4096)
        lib.hsrle_rle8_mmtf_tuning(1)
        assert lib.hsrle_rle8_mmtf128_blocks_workspace_size(0, 4096, 4096) > enc and lib.hsrle_rle8_mmtf128_blocks_workspace_size(1, 4096, 4096) == dec
    finally:
        lib.hsrle_rle8_mmtf128_blocks_tuning(0)
        lib.hsrle_rle8_mmtf_tuning(0)


def sample():
    data = T.random_alphabet(3 * 128 + 17, 3, 9)
    return data, B.build(data, 128)


def info_of(lib, container, size=None):
    info = Info()
    rc = lib.hsrle_rle8_mmtf128_blocks_info_host(bytes(container), len(container) if size is None else size, ctypes.byref(info))
    return rc, info


def test_info_host_reads_a_python_built_container(lib):
    data, c = sample()
    rc, info = info_of(lib, c)
    assert rc == OK
    h = B.header(c)
    assert (info.uncompressedSize, info.blockSize, info.blockCount, info.payloadSize, info.totalSize) == (len(data), 128, 4, h["payloadSize"], len(c))
    assert info_of(lib, c + bytes(100))[0] == OK                                            # a buffer larger than the container
    assert info_of(lib, c, len(c) - 1)[0] == ERR_FORMAT                                     # totalSize above the buffer
    assert info_of(lib, c, 63)[0] == ERR_ARGUMENT
    assert lib.hsrle_rle8_mmtf128_blocks_info_host(None, 1000, ctypes.byref(info)) == ERR_ARGUMENT
    assert lib.hsrle_rle8_mmtf128_blocks_info_host(bytes(c), len(c), None) == ERR_ARGUMENT
    i2 = hsrle.rle8_mmtf128_blocks_info(c)
    assert isinstance(i2, Info) and (i2.uncompressedSize, i2.totalSize) == (len(data), len(c))


BROKEN_FIELDS = {
    "magic": (0, b"HSRLEMFb"),
    "version_0": (8, struct.pack("<I", 0)),
    "version_2": (8, struct.pack("<I", 2)),
    "reserved": (12, struct.pack("<I", 1)),
    "uncompressed_size_0": (16, struct.pack("<Q", 0)),
    "uncompressed_size_one_block_more": (16, struct.pack("<Q", 4 * 128 + 1)),
    "uncompressed_size_one_block_less": (16, struct.pack("<Q", 3 * 128)),
    "block_size_0": (24, struct.pack("<I", 0)),
    "block_size_not_a_multiple_of_128": (24, struct.pack("<I", 192)),
    "block_size_64": (24, struct.pack("<I", 64)),
    "block_size_above_2_to_the_20": (24, struct.pack("<I", (1 << 20) + 128)),
    "block_count_less": (28, struct.pack("<I", 3)),
    "block_count_more": (28, struct.pack("<I", 5)),
    "payload_size_more": (32, None),
    "payload_size_huge": (32, struct.pack("<Q", (1 << 64) - 40)),
    "total_size_less": (40, None),
    "zero_first": (48, b"\x01"),
    "zero_last": (63, b"\x80"),
}


@pytest.mark.parametrize("name", list(BROKEN_FIELDS))
def test_info_host_refuses_a_broken_header_field(lib, name):
    _, c = sample()
    at, patch = BROKEN_FIELDS[name]
    if name == "payload_size_more":
        patch = struct.pack("<Q", B.header(c)["payloadSize"] + 1)
    if name == "total_size_less":
        patch = struct.pack("<Q", len(c) - 1)
    bad = c[:at] + patch + c[at + len(patch) :]
    assert bad != c
    assert info_of(lib, bad + bytes(4096))[0] == ERR_FORMAT, name
    assert info_of(lib, c + bytes(4096))[0] == OK


def test_the_three_families_refuse_each_others_magics(lib):
    _, c = sample()
    kit, shb = KitInfo(), Info()
    sh_info = lambda x: lib.hsrle_rle8_sh_blocks_info_host(bytes(x), len(x), ctypes.byref(shb))        # noqa: E731
    kit_info = lambda x: lib.hsrle_container_info_host(bytes(x), len(x), ctypes.byref(kit))            # noqa: E731
    assert B.MAGIC == b"HSRLEMFB" and SHB.MAGIC == b"HSRLESHB"
    # this container under its own magic: only its own family reads it
    assert info_of(lib, c)[0] == OK and sh_info(c) == ERR_FORMAT and kit_info(c) == ERR_FORMAT
    # the same header lines under the other families' magics
    assert info_of(lib, SHB.MAGIC + c[8:])[0] == ERR_FORMAT and sh_info(SHB.MAGIC + c[8:]) == OK
    assert info_of(lib, b"HSRLEKIT" + c[8:])[0] == ERR_FORMAT
    # a section-2 header as it stands (codec 0, 4 blocks of 128)
    payload = 40
    sect2 = b"HSRLEKIT" + struct.pack("<IIQIIQQ", 1, 0, 4 * 128, 128, 4, payload, 64 + 8 * 5 + payload + 32) + bytes(16) + bytes(8 * 5 + payload + 32)
    assert kit_info(sect2) == OK
    assert info_of(lib, sect2)[0] == ERR_FORMAT and sh_info(sect2) == ERR_FORMAT
    assert kit_info(B.MAGIC + sect2[8:]) == ERR_FORMAT


def test_host_calls_refuse_on_the_host(lib):
    _, c = sample()
    src, dst = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(8192)
    a, b = ctypes.addressof(src), ctypes.addressof(dst)
    size = ctypes.c_uint64(7)
    C, D = lib.hsrle_rle8_mmtf128_compress_blocks_host, lib.hsrle_rle8_mmtf128_decompress_blocks_host
    assert C(None, 1024, 128, b, 8192, ctypes.byref(size)) == ERR_ARGUMENT
    assert C(a, 1024, 128, None, 8192, ctypes.byref(size)) == ERR_ARGUMENT
    assert C(a, 0, 128, b, 8192, ctypes.byref(size)) == ERR_ARGUMENT
    assert C(a, 1024, 100, b, 8192, ctypes.byref(size)) == ERR_ARGUMENT
    assert D(None, 1000, b, 8192, ctypes.byref(size)) == ERR_ARGUMENT
    assert D(bytes(c), 63, b, 8192, ctypes.byref(size)) == ERR_ARGUMENT
    assert D(b"HSRLEKIT" + c[8:], len(c), b, 8192, ctypes.byref(size)) == ERR_FORMAT
    assert D(SHB.MAGIC + c[8:], len(c), b, 8192, ctypes.byref(size)) == ERR_FORMAT
    assert D(bytes(c), len(c), b, 3 * 128 + 16, ctypes.byref(size)) == ERR_CAPACITY         # outCapacity < uncompressedSize
    assert D(bytes(c), len(c), None, 8192, ctypes.byref(size)) == ERR_CAPACITY
    assert size.value == 7 and dst.raw == bytes(8192)


def test_dev_async_argument_checks(lib):
    # host buffers stand in for device pointers: every call below is refused on the host, before anything could touch them
    src, dst, ws, words = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(8192), ctypes.create_string_buffer(64), ctypes.create_string_buffer(32)
    a, b, w, s = ctypes.addressof(src), ctypes.addressof(dst), ctypes.addressof(ws), (ctypes.addressof(words) + 7) & ~7
    big = 1 << 40
    C, D = lib.hsrle_rle8_mmtf128_compress_blocks_dev_async, lib.hsrle_rle8_mmtf128_decompress_blocks_dev_async
    n, bs = 1024, 128
    need = lib.hsrle_rle8_mmtf128_blocks_workspace_size(0, n, bs)
    least = 64 + 8 * 9 + 32                                                                 # header + table + pad of 8 blocks
    assert C(None, n, bs, b, 4096, s, s + 8, w, big, None) == ERR_ARGUMENT
    assert C(a, n, bs, None, 4096, s, s + 8, w, big, None) == ERR_ARGUMENT
    assert C(a, n, bs, b, 4096, None, s + 8, w, big, None) == ERR_ARGUMENT
    assert C(a, n, bs, b, 4096, s, None, w, big, None) == ERR_ARGUMENT
    assert C(a, n, bs, b, 4096, s, s + 8, None, big, None) == ERR_ARGUMENT
    for bad in (64, 192, 127, (1 << 20) + 128):
        assert C(a, n, bad, b, 4096, s, s + 8, w, big, None) == ERR_ARGUMENT, bad           # a bad block size
    assert C(a, 0, bs, b, 4096, s, s + 8, w, big, None) == ERR_ARGUMENT
    assert C(a, (128 << 32) + 1, bs, a + (1 << 50), big, s, s + 8, w, big, None) == ERR_ARGUMENT   # a block count that does not fit 32 bits
    assert C(a, n, bs, a + 1000, 4096, s, s + 8, w, big, None) == ERR_ARGUMENT              # overlap
    assert C(a + 100, n, bs, a, 101, s, s + 8, w, big, None) == ERR_ARGUMENT                # overlap by one byte of the capacity
    assert C(a, n, bs, b, 4096, s + 4, s + 8, w, big, None) == ERR_ARGUMENT                 # the size word is 8 bytes: 8-byte aligned
    assert C(a, n, bs, b, 4096, s, s + 10, w, big, None) == ERR_ARGUMENT                    # unaligned status word
    assert C(a, n, bs, a + 1000, least - 1, s + 4, s + 8, w, 0, None) == ERR_ARGUMENT       # arguments are judged in front of the capacities
    assert C(a, n, bs, b, least - 1, s, s + 8, w, big, None) == ERR_CAPACITY                # cannot hold even header + table + pad
    assert C(a, n, bs, b, 4096, s, s + 8, w, need - 1, None) == ERR_CAPACITY
    assert C(a, n, 0, b, 4096, s, s + 8, w, lib.hsrle_rle8_mmtf128_blocks_workspace_size(0, n, 4096) - 1, None) == ERR_CAPACITY   # block size 0: 4096

    _, c = sample()
    good = info_of(lib, c)[1]
    need = lib.hsrle_rle8_mmtf128_blocks_workspace_size(1, 4 * 128, 128)

    def info(**changes):
        i = Info(good.uncompressedSize, good.blockSize, good.blockCount, good.payloadSize, good.totalSize)
        for k, v in changes.items():
            setattr(i, k, v)
        return ctypes.byref(i)

    U = good.uncompressedSize
    assert D(None, info(), 0, 4, b, U, s, w, big, None) == ERR_ARGUMENT
    assert D(a, None, 0, 4, b, U, s, w, big, None) == ERR_ARGUMENT
    assert D(a, info(), 0, 4, None, U, s, w, big, None) == ERR_ARGUMENT
    assert D(a, info(), 0, 4, b, U, None, w, big, None) == ERR_ARGUMENT
    assert D(a, info(), 0, 4, b, U, s, None, big, None) == ERR_ARGUMENT
    for changes in ({"blockSize": 192}, {"blockSize": 0}, {"blockCount": 5}, {"uncompressedSize": 0}, {"totalSize": good.totalSize + 1}, {"payloadSize": good.payloadSize + 8}):
        assert D(a, info(**changes), 0, 1, b, 8192, s, w, big, None) == ERR_ARGUMENT, changes   # an info that contradicts itself
    assert D(a, info(), 0, 0, b, U, s, w, big, None) == ERR_ARGUMENT                        # a range of no blocks
    assert D(a, info(), 0, 5, b, U, s, w, big, None) == ERR_ARGUMENT                        # a range outside the container
    assert D(a, info(), 4, 1, b, U, s, w, big, None) == ERR_ARGUMENT
    assert D(a, info(), 3, 2, b, U, s, w, big, None) == ERR_ARGUMENT
    assert D(a, info(), 0xFFFFFFFF, 2, b, U, s, w, big, None) == ERR_ARGUMENT               # (first + count wraps in 32 bits)
    assert D(a, info(), 0, 5, b, U - 1, s, w, 0, None) == ERR_ARGUMENT                      # a bad range is judged in front of the capacities
    assert D(a, info(), 0, 4, b, U - 1, s, w, big, None) == ERR_CAPACITY                    # outCapacity < uncompressedSize
    assert D(a, info(), 1, 2, b, 2 * 128, s, w, big, None) == ERR_CAPACITY                  # ... also for a range: blocks land at i * blockSize
    assert D(a, info(), 0, 4, a + good.totalSize - 1, U, s, w, big, None) == ERR_ARGUMENT   # overlap
    assert D(a, info(), 0, 4, b, U, s + 2, w, big, None) == ERR_ARGUMENT                    # unaligned status word
    assert D(a, info(), 0, 4, b, U, s, w, need - 1, None) == ERR_CAPACITY
    assert D(a, info(), 1, 2, b, U, s, w, lib.hsrle_rle8_mmtf128_blocks_workspace_size(1, 2 * 128, 128) - 1, None) == ERR_CAPACITY   # a range needs its own blocks' slots
    assert dst.raw == bytes(8192) and words.raw == bytes(32)
