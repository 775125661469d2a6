"""Which rule wins where a call to a stream codec's entry breaks two at once: the seven _dev_async entries of rle8_sh, rle8_mmtf128, the mmtf transforms and
the rle8_sh block container, and the container's two _host calls.  The ABI tests break one rule per call; the order of the checks shows only here.  The codes
below are the ones the build before the shared entry check (csrc/hsrle_capi_host.h) returned, as literals.  Host buffers stand in for device pointers and
every call is refused on the host: nothing touches a device, and the destination stays as it was.

The combinations: a null pointer and a capacity too small; an overlap and a capacity too small; a misaligned status word and a workspace too small; a bad
size and an overlap.  The single-stream decoders have no output capacity of their own (the output size is the plan's), so their capacity is the workspace's;
hsrle_mmtf_dev_async has no status word; the _host calls test neither overlap nor alignment, so they pair what they do test."""
import ctypes
import os

import pytest

import hsrle
import rle8_sh_blocks_testlib as B
import rle8_sh_testlib as T

OK, ERR_ARGUMENT, ERR_CAPACITY, ERR_FORMAT = 0, 1, 2, 3
MAX_IN = 1 << 30
BIG = 1 << 40


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(hsrle.LIB_PATH):
        import subprocess

        subprocess.check_call(["make", "-s", "-j8", "-C", hsrle.PKG_DIR])
    L = ctypes.CDLL(hsrle.LIB_PATH)
    hsrle.declare(L)
    return L


class Buffers:
    def __init__(self):
        self.src, self.dst = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(8192)
        self.ws, self.words = ctypes.create_string_buffer(64), ctypes.create_string_buffer(32)
        self.a, self.b, self.w = ctypes.addressof(self.src), ctypes.addressof(self.dst), ctypes.addressof(self.ws)
        self.s = (ctypes.addressof(self.words) + 7) & ~7

    def untouched(self):
        return self.dst.raw == bytes(8192) and self.words.raw == bytes(32) and self.ws.raw == bytes(64) and self.src.raw == bytes(4096)


def single_stream_cases(L, family):
    """(id, call) of hsrle_<family>_compress_dev_async / _decompress_dev_async"""
    C, D = getattr(L, f"hsrle_{family}_compress_dev_async"), getattr(L, f"hsrle_{family}_decompress_dev_async")
    W = getattr(L, f"hsrle_{family}_workspace_size")
    enc, dec = W(0, 1024), W(1, 1024)
    return [
        ("compress: null input, output capacity too small", lambda m: C(None, 1024, m.b, 1024 + 7, m.s, m.s + 4, m.w, BIG, None)),
        ("compress: null workspace, workspace too small", lambda m: C(m.a, 1024, m.b, 2048, m.s, m.s + 4, None, enc - 1, None)),
        ("compress: overlap, output capacity too small", lambda m: C(m.a + 100, 1024, m.a, 101, m.s, m.s + 4, m.w, BIG, None)),
        ("compress: overlap, workspace too small", lambda m: C(m.a, 1024, m.a + 1000, 2048, m.s, m.s + 4, m.w, enc - 1, None)),
        ("compress: misaligned status, workspace too small", lambda m: C(m.a, 1024, m.b, 2048, m.s, m.s + 6, m.w, enc - 1, None)),
        ("compress: misaligned size word, output capacity too small", lambda m: C(m.a, 1024, m.b, 1024 + 7, m.s + 1, m.s + 4, m.w, BIG, None)),
        ("compress: size 0, overlap", lambda m: C(m.a, 0, m.a, 2048, m.s, m.s + 4, m.w, BIG, None)),
        ("compress: size above 2^30, overlap", lambda m: C(m.a, MAX_IN + 1, m.a + 1000, BIG, m.s, m.s + 4, m.w, BIG, None)),
        ("compress: size above 2^30, output capacity too small", lambda m: C(m.a, MAX_IN + 1, m.b, 16, m.s, m.s + 4, m.w, BIG, None)),
        ("decompress: null stream, workspace too small", lambda m: D(None, 100, m.b, 1024, m.s, m.w, dec - 1, None)),
        ("decompress: overlap, workspace too small", lambda m: D(m.a, 100, m.a + 50, 1024, m.s, m.w, dec - 1, None)),
        ("decompress: misaligned status, workspace too small", lambda m: D(m.a, 100, m.b, 1024, m.s + 2, m.w, dec - 1, None)),
        ("decompress: stream size 0, overlap", lambda m: D(m.a, 0, m.a, 1024, m.s, m.w, BIG, None)),
        ("decompress: output size above 2^30, overlap", lambda m: D(m.a, 100, m.a + 50, MAX_IN + 1, m.s, m.w, BIG, None)),
        ("decompress: output size 0, workspace too small", lambda m: D(m.a, 100, m.b, 0, m.s, m.w, 0, None)),
    ]


def mmtf_cases(L):
    M, need = L.hsrle_mmtf_dev_async, L.hsrle_mmtf_workspace_size(0, 32)
    return [
        ("null input, workspace too small", lambda m: M(0, 0, None, 32, m.b, m.w, need - 1, None)),
        ("overlap, workspace too small", lambda m: M(0, 1, m.a, 32, m.a + 31, m.w, need - 1, None)),
        ("unknown transform, overlap", lambda m: M(4, 0, m.a, 32, m.a, m.w, BIG, None)),
        ("size 2^32, overlap", lambda m: M(0, 0, m.a, 1 << 32, m.a, m.w, BIG, None)),
        ("size 2^32, null output", lambda m: M(1, 0, m.a, 1 << 32, None, m.w, BIG, None)),
        ("size 0, null pointers, no workspace", lambda m: M(2, 1, None, 0, None, None, 0, None)),
        ("size 0, unknown transform", lambda m: M(-1, 1, m.a, 0, m.b, m.w, BIG, None)),
    ]


def sample():
    data = T.geometric_runs(3 * 128 + 17, 4, 9)
    return data, B.build(data, 128)


def blocks_dev_cases(L):
    C, D = L.hsrle_rle8_sh_compress_blocks_dev_async, L.hsrle_rle8_sh_decompress_blocks_dev_async
    n, bs = 1024, 128
    enc = L.hsrle_rle8_sh_blocks_workspace_size(0, n, bs)
    least = 64 + 8 * 9 + 32
    _, c = sample()
    good = hsrle.Rle8ShBlocksInfo()
    assert L.hsrle_rle8_sh_blocks_info_host(bytes(c), len(c), ctypes.byref(good)) == OK
    U, dec = good.uncompressedSize, L.hsrle_rle8_sh_blocks_workspace_size(1, good.uncompressedSize, 128)

    def info(**changes):
        i = hsrle.Rle8ShBlocksInfo(good.uncompressedSize, good.blockSize, good.blockCount, good.payloadSize, good.totalSize)
        for k, v in changes.items():
            setattr(i, k, v)
        return ctypes.byref(i)

    return [
        ("compress: null input, output capacity too small", lambda m: C(None, n, bs, m.b, least - 1, m.s, m.s + 8, m.w, BIG, None)),
        ("compress: null status, workspace too small", lambda m: C(m.a, n, bs, m.b, 4096, m.s, None, m.w, enc - 1, None)),
        ("compress: overlap, output capacity too small", lambda m: C(m.a + 100, n, bs, m.a, 101, m.s, m.s + 8, m.w, BIG, None)),
        ("compress: overlap, workspace too small", lambda m: C(m.a, n, bs, m.a + 1000, 4096, m.s, m.s + 8, m.w, enc - 1, None)),
        ("compress: misaligned status, workspace too small", lambda m: C(m.a, n, bs, m.b, 4096, m.s, m.s + 10, m.w, enc - 1, None)),
        ("compress: misaligned size word, output capacity too small", lambda m: C(m.a, n, bs, m.b, least - 1, m.s + 4, m.s + 8, m.w, BIG, None)),
        ("compress: size 0, overlap", lambda m: C(m.a, 0, bs, m.a, 4096, m.s, m.s + 8, m.w, BIG, None)),
        ("compress: bad block size, overlap", lambda m: C(m.a, n, 192, m.a + 1000, 4096, m.s, m.s + 8, m.w, BIG, None)),
        ("compress: bad block size, output capacity too small", lambda m: C(m.a, n, 64, m.b, 16, m.s, m.s + 8, m.w, BIG, None)),
        ("decompress: null container, output capacity too small", lambda m: D(None, info(), 0, 4, m.b, U - 1, m.s, m.w, BIG, None)),
        ("decompress: null workspace, workspace too small", lambda m: D(m.a, info(), 0, 4, m.b, U, m.s, None, dec - 1, None)),
        ("decompress: overlap, output capacity too small", lambda m: D(m.a, info(), 0, 4, m.a + good.totalSize - 1, U - 1, m.s, m.w, BIG, None)),
        ("decompress: overlap, workspace too small", lambda m: D(m.a, info(), 0, 4, m.a + good.totalSize - 1, U, m.s, m.w, dec - 1, None)),
        ("decompress: misaligned status, workspace too small", lambda m: D(m.a, info(), 0, 4, m.b, U, m.s + 2, m.w, dec - 1, None)),
        ("decompress: misaligned status, output capacity too small", lambda m: D(m.a, info(), 0, 4, m.b, U - 1, m.s + 2, m.w, BIG, None)),
        ("decompress: inconsistent info, overlap", lambda m: D(m.a, info(blockCount=5), 0, 1, m.a, 8192, m.s, m.w, BIG, None)),
        ("decompress: uncompressed size 0, output capacity too small", lambda m: D(m.a, info(uncompressedSize=0), 0, 1, m.b, 0, m.s, m.w, BIG, None)),
        ("decompress: range outside the container, overlap", lambda m: D(m.a, info(), 3, 2, m.a, U, m.s, m.w, BIG, None)),
        ("decompress: range of no blocks, output capacity too small", lambda m: D(m.a, info(), 0, 0, m.b, U - 1, m.s, m.w, BIG, None)),
    ]


def blocks_host_cases(L):
    C, D = L.hsrle_rle8_sh_compress_blocks_host, L.hsrle_rle8_sh_decompress_blocks_host
    _, c = sample()
    size = ctypes.c_uint64(7)
    z = ctypes.byref(size)
    return [
        ("compress: null input, output capacity too small", lambda m: C(None, 1024, 128, m.b, 16, z)),
        ("compress: null output, output capacity 0", lambda m: C(m.a, 1024, 128, None, 0, z)),
        ("compress: size 0, overlap", lambda m: C(m.a, 0, 128, m.a, 8192, z)),
        ("compress: bad block size, output capacity too small", lambda m: C(m.a, 1024, 100, m.b, 16, z)),
        ("compress: bad block size, overlap", lambda m: C(m.a, 1024, 192, m.a + 1000, 8192, z)),
        ("decompress: null container, output capacity too small", lambda m: D(None, 1000, m.b, 16, z)),
        ("decompress: container below a header, null output", lambda m: D(bytes(c), 63, None, 0, z)),
        ("decompress: another magic, output capacity too small", lambda m: D(b"HSRLEKIT" + c[8:], len(c), m.b, 16, z)),
        ("decompress: another magic, null output", lambda m: D(b"HSRLEKIT" + c[8:], len(c), None, 8192, z)),
        ("decompress: null output, output capacity too small", lambda m: D(bytes(c), len(c), None, 16, z)),
        ("decompress: total size above the buffer, output capacity too small", lambda m: D(bytes(c), len(c) - 1, m.b, 16, z)),
    ]


ENTRIES = {
    "rle8_sh": lambda L: single_stream_cases(L, "rle8_sh"),
    "rle8_mmtf128": lambda L: single_stream_cases(L, "rle8_mmtf128"),
    "mmtf": mmtf_cases,
    "rle8_sh_blocks_dev": blocks_dev_cases,
    "rle8_sh_blocks_host": blocks_host_cases,
}

A, CAP, FMT = ERR_ARGUMENT, ERR_CAPACITY, ERR_FORMAT
EXPECTED = {
    "rle8_sh": {
        "compress: null input, output capacity too small": A,
        "compress: null workspace, workspace too small": A,
        "compress: overlap, output capacity too small": A,
        "compress: overlap, workspace too small": A,
        "compress: misaligned status, workspace too small": A,
        "compress: misaligned size word, output capacity too small": A,
        "compress: size 0, overlap": A,
        "compress: size above 2^30, overlap": A,
        "compress: size above 2^30, output capacity too small": A,
        "decompress: null stream, workspace too small": A,
        "decompress: overlap, workspace too small": A,
        "decompress: misaligned status, workspace too small": A,
        "decompress: stream size 0, overlap": A,
        "decompress: output size above 2^30, overlap": A,
        "decompress: output size 0, workspace too small": A,
    },
    "rle8_mmtf128": {
        "compress: null input, output capacity too small": A,
        "compress: null workspace, workspace too small": A,
        "compress: overlap, output capacity too small": A,
        "compress: overlap, workspace too small": A,
        "compress: misaligned status, workspace too small": A,
        "compress: misaligned size word, output capacity too small": A,
        "compress: size 0, overlap": A,
        "compress: size above 2^30, overlap": A,
        "compress: size above 2^30, output capacity too small": A,
        "decompress: null stream, workspace too small": A,
        "decompress: overlap, workspace too small": A,
        "decompress: misaligned status, workspace too small": A,
        "decompress: stream size 0, overlap": A,
        "decompress: output size above 2^30, overlap": A,
        "decompress: output size 0, workspace too small": A,
    },
    "mmtf": {
        "null input, workspace too small": A,
        "overlap, workspace too small": A,
        "unknown transform, overlap": A,
        "size 2^32, overlap": A,
        "size 2^32, null output": A,
        "size 0, null pointers, no workspace": OK,
        "size 0, unknown transform": A,
    },
    "rle8_sh_blocks_dev": {
        "compress: null input, output capacity too small": A,
        "compress: null status, workspace too small": A,
        "compress: overlap, output capacity too small": A,
        "compress: overlap, workspace too small": A,
        "compress: misaligned status, workspace too small": A,
        "compress: misaligned size word, output capacity too small": A,
        "compress: size 0, overlap": A,
        "compress: bad block size, overlap": A,
        "compress: bad block size, output capacity too small": A,
        "decompress: null container, output capacity too small": A,
        "decompress: null workspace, workspace too small": A,
        "decompress: overlap, output capacity too small": CAP,
        "decompress: overlap, workspace too small": A,
        "decompress: misaligned status, workspace too small": A,
        "decompress: misaligned status, output capacity too small": CAP,
        "decompress: inconsistent info, overlap": A,
        "decompress: uncompressed size 0, output capacity too small": A,
        "decompress: range outside the container, overlap": A,
        "decompress: range of no blocks, output capacity too small": A,
    },
    "rle8_sh_blocks_host": {
        "compress: null input, output capacity too small": A,
        "compress: null output, output capacity 0": A,
        "compress: size 0, overlap": A,
        "compress: bad block size, output capacity too small": A,
        "compress: bad block size, overlap": A,
        "decompress: null container, output capacity too small": A,
        "decompress: container below a header, null output": A,
        "decompress: another magic, output capacity too small": FMT,
        "decompress: another magic, null output": FMT,
        "decompress: null output, output capacity too small": CAP,
        "decompress: total size above the buffer, output capacity too small": FMT,
    },
}


def observed(L, entry):
    """[(case id, return code, every buffer untouched)] of one entry's cases, each on fresh buffers"""
    out = []
    for name, call in ENTRIES[entry](L):
        m = Buffers()
        rc = call(m)
        out.append((name, rc, m.untouched()))
    return out


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_the_first_broken_rule_in_the_entrys_order_decides(lib, entry):
    got = observed(lib, entry)
    assert [name for name, _, _ in got] == list(EXPECTED[entry]), "the cases and the recorded codes must be the same list"
    for name, rc, untouched in got:
        assert rc == EXPECTED[entry][name], f"{entry}: {name}"
        assert untouched, f"{entry}: {name}: a refused call wrote to a buffer"
