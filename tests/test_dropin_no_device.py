"""The host-pointer drop-in functions check their arguments -- and whether there is a device at all -- before they touch memory: one function of every
family (monolithic codecs, rle8m, the unsectioned low-entropy codec, its three split-phase helpers that use the device), each with valid arguments and
with each pointer argument NULL in turn, plus decompress_with_info with a symbolToCount that is no permutation.  A NULL pointer gives 0 / false with
or without a device.  Valid arguments give 0 / false where hsrle_device_count() is 0 (the machines that run this suite without a GPU: nothing is staged,
nothing crashes) and a result where there is one.  This pins the order of the checks in front of the shared staging (csrc/hsrle_capi_dropin.h)."""
import ctypes
import os
import random

import pytest

import hsrle

from hsrle_testlib import CODEC_BY_KEY, mixed_runs

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hypersonic-rle-kit_amd", "libhsrle_hip.so")


class CompressInfo(ctypes.Structure):
    _fields_ = [("rle", ctypes.c_uint8 * 256), ("symbolsByProb", ctypes.c_uint8 * 256), ("symbolCount", ctypes.c_uint8)]


class DecompressInfo(ctypes.Structure):
    _fields_ = [("rle", ctypes.c_uint8 * 256), ("symbolToCount", ctypes.c_uint8 * 256)]


@pytest.fixture(scope="module")
def lib():
    return hsrle.declare(ctypes.CDLL(LIB))                            # (a missing library is a failed build: an error, not a skip)


def _check(fn, args, pointers, succeeds):
    """fn(*args) gives a result exactly where `succeeds`; with any of the arguments at `pointers` NULL it gives 0 / false"""
    assert bool(fn(*args)) == succeeds, f"{fn.__name__} with valid arguments"
    for k in pointers:
        nulled = list(args)
        nulled[k] = None
        assert not fn(*nulled), f"{fn.__name__} with argument {k} NULL"


def test_every_dropin_family_refuses_without_touching_memory(lib, oracle):
    has_device = lib.hsrle_device_count() > 0
    data = mixed_runs(random.Random(9), 5000, alphabet=3)
    n = len(data)
    src = ctypes.create_string_buffer(data, n + 512)
    out = ctypes.create_string_buffer(2 * n + 4096)

    def staged(stream):
        return ctypes.create_string_buffer(stream, len(stream) + 512)

    # the monolithic codecs
    stream = oracle.compress(CODEC_BY_KEY["rle8_multi"], data)
    _check(lib.rle8_multi_compress, [src, n, out, lib.rle_compress_bounds(n)], (0, 2), has_device)
    _check(lib.rle8_decompress, [staged(stream), len(stream), out, n], (0, 2), has_device)
    # rle8m
    stream = oracle.rle8m_compress(7, data)
    _check(lib.rle8m_compress, [7, src, n, out, lib.rle8m_compress_bounds(7, n)], (1, 3), has_device)
    _check(lib.rle8m_decompress, [staged(stream), len(stream), out, n], (0, 2), has_device)
    # the unsectioned low-entropy codec
    stream = oracle.low_entropy_compress(0, data)
    _check(lib.rle8_low_entropy_compress, [src, n, out, lib.rle8_low_entropy_compress_bounds(n)], (0, 2), has_device)
    _check(lib.rle8_low_entropy_decompress, [staged(stream), len(stream), out, n], (0, 2), has_device)
    # ... and its split-phase helpers that use the device
    info = CompressInfo()
    _check(lib.rle8_low_entropy_get_compress_info, [src, n, ctypes.byref(info)], (0, 2), has_device)
    if not has_device:                                                 # (tables of the test's own: any permutation will do)
        for k in range(256):
            info.symbolsByProb[k] = k
        info.symbolCount = 3
    _check(lib.rle8_low_entropy_compress_with_info, [src, n, ctypes.byref(info), out, 2 * n + 600], (0, 2, 3), has_device)
    dinfo = DecompressInfo()
    hsize = lib.rle8_low_entropy_read_decompress_info(stream[8:], len(stream) - 8, ctypes.byref(dinfo))
    assert hsize == 33 + (stream[8 + 32] or 255)
    body = staged(stream[8 + hsize :])
    first = ctypes.addressof(body)
    end = first + len(stream) - 8 - hsize
    _check(lib.rle8_low_entropy_decompress_with_info, [first, end, ctypes.byref(dinfo), out, n], (0, 1, 2, 3), has_device)
    if has_device:
        assert out.raw[:n] == data
    bad = DecompressInfo()                                             # every count 0: no permutation
    assert lib.rle8_low_entropy_decompress_with_info(first, end, ctypes.byref(bad), out, n) == 0
