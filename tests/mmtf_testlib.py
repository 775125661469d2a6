"""Helpers of the mmtf / bitmmtf tests: the sequential definition of the four transforms (reference: src/mmtf.c, src/bit_mmtf.c, src/rle.h:420-438),
a small ctypes wrapper of the compiled reference (optional: oracle/_ref/libhsrle_ref.so), and the inputs the tests share."""
import ctypes
import os
import random

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(REPO, "oracle", "_ref", "libhsrle_ref.so")
GOLDEN_DIR = os.path.join(REPO, "tests", "golden", "mmtf")

MMTF128, MMTF256, BITMMTF8, BITMMTF16 = range(4)
TRANSFORMS = (MMTF128, MMTF256, BITMMTF8, BITMMTF16)
NAMES = {MMTF128: "mmtf128", MMTF256: "mmtf256", BITMMTF8: "bitmmtf8", BITMMTF16: "bitmmtf16"}
WIDTH = {MMTF128: 16, MMTF256: 32, BITMMTF8: 16, BITMMTF16: 16}   # (for the bit transforms: only what the size lists are built around)


def mmtf_enc(data, W):
    n = len(data)
    rows = n // W
    out = bytearray(n)
    lists = [list(range(256)) for _ in range(W)]
    for i in range(rows * W):
        l = lists[i % W]
        k = l.index(data[i])
        out[i] = k
        if k:
            l.insert(0, l.pop(k))
    for i in range(rows * W, n):                 # tail of n % W bytes: rank in column (i - rows * W)'s list, list NOT updated
        out[i] = lists[i - rows * W].index(data[i])
    return bytes(out)


def mmtf_dec(data, W):
    n = len(data)
    rows = n // W
    out = bytearray(n)
    lists = [list(range(256)) for _ in range(W)]
    for i in range(rows * W):
        l = lists[i % W]
        k = data[i]
        out[i] = l[k]
        if k:
            l.insert(0, l.pop(k))
    for i in range(rows * W, n):
        out[i] = lists[i - rows * W][data[i]]
    return bytes(out)


def bitmmtf_enc(data, E):
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    m = len(a) & ~(E - 1)
    out = a.copy()
    out[E:m] = a[E:m] ^ a[: m - E]
    return out.tobytes()


def bitmmtf_dec(data, E):
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    m = len(a) & ~(E - 1)
    out = a.copy()
    for phase in range(E):
        out[phase:m:E] = np.bitwise_xor.accumulate(a[phase:m:E])
    return out.tobytes()


def model(transform, decode, data):
    data = bytes(data)
    if transform in (MMTF128, MMTF256):
        return (mmtf_dec if decode else mmtf_enc)(data, WIDTH[transform])
    return (bitmmtf_dec if decode else bitmmtf_enc)(data, 1 if transform == BITMMTF8 else 2)


def function_name(transform, decode):
    return NAMES[transform] + ("_decode" if decode else "_encode")


class MmtfReference:
    """The ten functions of the compiled reference.  Buffers get 64 bytes of slack; `misalign` shifts both pointers off their 64-byte
    alignment (the reference dispatches on the pointers' alignment: both branches must give the same bytes)."""

    @staticmethod
    def available():
        return os.path.exists(REF_LIB)

    def __init__(self):
        self.lib = ctypes.CDLL(REF_LIB)
        for t in TRANSFORMS:
            for d in (0, 1):
                f = getattr(self.lib, function_name(t, d))
                f.restype = ctypes.c_uint32
                f.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
        for nm in ("mmtf_bounds", "bitmmtf_bounds"):
            f = getattr(self.lib, nm)
            f.restype = ctypes.c_uint32
            f.argtypes = [ctypes.c_uint32]

    def bounds(self, name, n):
        return getattr(self.lib, name)(n)

    def run(self, transform, decode, data, misalign=0, out_size=None):
        """(return value, output bytes[:len(data)])"""
        data = bytes(data)
        n = len(data)
        cap = n if out_size is None else out_size
        src = ctypes.create_string_buffer(n + 192)
        dst = ctypes.create_string_buffer(max(n, cap) + 192)
        a = (ctypes.addressof(src) + 63) // 64 * 64 + misalign
        b = (ctypes.addressof(dst) + 63) // 64 * 64 + misalign
        ctypes.memmove(a, data, n)
        rc = getattr(self.lib, function_name(transform, decode))(a, n, b, cap)
        return rc, ctypes.string_at(b, n)


# ---- inputs ----

def random_bytes(n, alphabet, seed):
    rng = random.Random(seed * 1000003 + alphabet * 131 + n)
    if alphabet == 256:
        return rng.randbytes(n)
    return bytes(rng.randrange(alphabet) for _ in range(n))


def every_symbol_per_column(n, W):
    """Row r holds the value r % 256 in every column: every column meets all 256 symbols, rank 255 occurs, and symbols first appear in
    late segments."""
    return bytes((i // W) % 256 for i in range(n))


def late_symbols_in_some_columns(n, W, segment_rows):
    """Small alphabet everywhere; in the LAST segment of `segment_rows` rows the even columns meet symbols never seen before."""
    rng = random.Random(n * 7 + W)
    a = bytearray(rng.randrange(3) for _ in range(n))
    rows = n // W
    last = ((rows - 1) // segment_rows) * segment_rows if rows else 0
    for r in range(last, rows):
        for c in range(0, W, 2):
            a[r * W + c] = 200 + (r * 5 + c) % 50
    return bytes(a)


def video_shaped(n, seed=3):
    """Zero dominated, short bursts of small values (the shape of hsrle_synth's video workload, made on the host)."""
    rng = np.random.default_rng(seed)
    a = np.zeros(n, dtype=np.uint8)
    starts = rng.integers(0, max(n, 1), size=max(n // 64, 1))
    for s in starts:
        ln = int(rng.integers(1, 12))
        a[s : s + ln] = rng.integers(1, 16, size=len(a[s : s + ln]), dtype=np.uint8)
    return a.tobytes()


def sizes_for(W):
    return [1, W - 1, W, W + 1, 2 * W - 1, 64 * W, 64 * W + 5, 4096, 65536 + W + 3]
