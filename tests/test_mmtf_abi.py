"""The mmtf / bitmmtf exports without a GPU: the reference's names (src/rle.h:420-438: eight transform functions and two bounds) and the three hsrle_mmtf_* names are in the
library, the bounds, the workspace size's conditions (a design condition: the state table of the move-to-front transforms stays below an eighth of
the input), and the return values that are decided on the host before any device is touched."""
import ctypes
import os

import pytest

import hsrle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "hypersonic-rle-kit_amd", "libhsrle_hip.so")

REFERENCE_NAMES = ["mmtf_bounds", "bitmmtf_bounds"] + [f"{t}_{d}" for t in ("mmtf128", "mmtf256", "bitmmtf8", "bitmmtf16") for d in ("encode", "decode")]
OWN_NAMES = ["hsrle_mmtf_workspace_size", "hsrle_mmtf_dev_async", "hsrle_mmtf_tuning"]
OK, ERR_ARGUMENT, ERR_CAPACITY = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess

        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(REPO, "hypersonic-rle-kit_amd")])
    L = hsrle.declare(ctypes.CDLL(LIB))
    L.hsrle_mmtf_tuning(0)
    return L


def test_names_are_exported(lib):
    assert len(REFERENCE_NAMES) == 8 + 2          # every declaration of rle.h:420-438: eight transform functions and the two bounds
    for nm in REFERENCE_NAMES + OWN_NAMES:
        assert hasattr(lib, nm), nm


def test_bounds(lib):
    assert lib.mmtf_bounds(1000) == 1000
    assert lib.bitmmtf_bounds(1000) == 1000
    assert lib.mmtf_bounds(0) == 0 and lib.bitmmtf_bounds(0xFFFFFFFF) == 0xFFFFFFFF


def test_workspace_size_rejects(lib):
    assert lib.hsrle_mmtf_workspace_size(4, 1 << 20) == 0
    assert lib.hsrle_mmtf_workspace_size(-1, 1 << 20) == 0
    for t in range(4):
        assert lib.hsrle_mmtf_workspace_size(t, 1 << 32) == 0
        assert lib.hsrle_mmtf_workspace_size(t, (1 << 32) - 1) > 0


def test_workspace_size_stays_small(lib):
    gib = 1 << 30
    for t in (0, 1):
        ws = lib.hsrle_mmtf_workspace_size(t, gib)
        assert 0 < ws <= gib // 8 + (1 << 20), ws
    for t in (2, 3):
        assert 0 < lib.hsrle_mmtf_workspace_size(t, gib) <= 1 << 20


def test_workspace_size_is_monotone(lib):
    sizes = sorted(set([0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 65536, 65555, (1 << 32) - 1] + [(1 << k) + d for k in range(8, 32) for d in (-1, 0, 1, 12345)]
                       + [i * 1000003 for i in range(1, 4000, 7)]))
    sizes = [s for s in sizes if s < (1 << 32)]
    for t in range(4):
        last = 0
        for s in sizes:
            ws = lib.hsrle_mmtf_workspace_size(t, s)
            assert ws >= last and ws > 0, (t, s, ws, last)
            last = ws


def test_host_decided_return_values(lib):
    src, dst = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    a, b = ctypes.addressof(src), ctypes.addressof(dst)
    assert lib.mmtf128_encode(a, 32, b, 31) == 0
    for nm in REFERENCE_NAMES[2:]:
        f = getattr(lib, nm)
        assert f(a, 32, b, 31) == 0, nm          # inSize > outSize
        assert f(a, 0, b, 64) == 0, nm           # returns inSize
    assert lib.bitmmtf8_encode(None, 32, b, 64) == 0
    for nm in ("bitmmtf8_encode", "bitmmtf8_decode", "bitmmtf16_encode", "bitmmtf16_decode"):
        assert getattr(lib, nm)(None, 32, b, 64) == 0, nm
        assert getattr(lib, nm)(a, 32, None, 64) == 0, nm


def test_dev_async_argument_checks(lib):
    # host buffers stand in for device pointers: every call below is refused (or is a no-op) on the host, before anything could touch them
    src, dst, ws = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    a, b, w = ctypes.addressof(src), ctypes.addressof(dst), ctypes.addressof(ws)
    big = 1 << 30
    assert lib.hsrle_mmtf_dev_async(4, 0, a, 32, b, w, big, None) == ERR_ARGUMENT
    assert lib.hsrle_mmtf_dev_async(0, 0, a, 1 << 32, b, w, big, None) == ERR_ARGUMENT
    for t in range(4):
        for decode in (0, 1):
            assert lib.hsrle_mmtf_dev_async(t, decode, a, 0, b, w, 0, None) == OK          # size 0: nothing to do
            assert lib.hsrle_mmtf_dev_async(t, decode, None, 32, b, w, big, None) == ERR_ARGUMENT
            assert lib.hsrle_mmtf_dev_async(t, decode, a, 32, None, w, big, None) == ERR_ARGUMENT
            assert lib.hsrle_mmtf_dev_async(t, decode, a, 32, b, None, big, None) == ERR_ARGUMENT
            assert lib.hsrle_mmtf_dev_async(t, decode, a, 32, a, w, big, None) == ERR_ARGUMENT   # dOut == dIn
            assert lib.hsrle_mmtf_dev_async(t, decode, a, 32, a + 31, w, big, None) == ERR_ARGUMENT
            assert lib.hsrle_mmtf_dev_async(t, decode, a, 32, b, w, lib.hsrle_mmtf_workspace_size(t, 32) - 1, None) == ERR_CAPACITY
