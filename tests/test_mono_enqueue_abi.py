"""hsrle_compress_mono_dev_enqueue without a GPU: the symbol is exported, and the codec set is decided on the host before anything else --
UNSUPPORTED for every codec whose encoder state at a cut is not fixed by the cut (lists of 3 / 7 symbols, Single, 128 bit, Greedy), and for
the 44 it takes an error that names the real problem (no device / no workspace), never UNSUPPORTED.  Nothing is enqueued in any of these calls."""
import ctypes
import os

import pytest

import hsrle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "hypersonic-rle-kit_amd", "libhsrle_hip.so")

OK, ERR_ARGUMENT, ERR_CAPACITY, ERR_FORMAT, ERR_DEVICE, ERR_UNSUPPORTED = range(6)
CODEC_COUNT = 110


def in_scope_names():
    names = {"rle8_multi", "rle8_packed_multi", "rle8_multi_short", "rle8_1symlut_short"}
    for W in (16, 24, 32, 48, 64):
        for v in ("sym", "byte"):
            names |= {f"rle{W}_{v}", f"rle{W}_{v}_packed", f"rle{W}_{v}_short", f"rle{W}_1symlut_{v}_short"}
    return names


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess

        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(REPO, "hypersonic-rle-kit_amd")])
    return hsrle.declare(ctypes.CDLL(LIB))


def codec_names(lib):
    return {i: lib.hsrle_codec_name(i).decode() for i in range(CODEC_COUNT)}


def enqueue(lib, codec, n=1 << 20, workspace_size=0, status=True):
    # host buffers stand in for device pointers: every call below is refused on the host, before anything could touch them
    src, dst, ws, word = (ctypes.create_string_buffer(16) for _ in range(4))
    return lib.hsrle_compress_mono_dev_enqueue(codec, ctypes.addressof(src), n, ctypes.addressof(dst), lib.rle_compress_bounds(n) + 64, ctypes.addressof(ws),
                                               workspace_size, None, ctypes.addressof(word) if status else None, None)


def test_symbol_is_exported(lib):
    assert hasattr(lib, "hsrle_compress_mono_dev_enqueue")


def test_the_scope_is_44_codecs(lib):
    names = set(codec_names(lib).values())
    assert in_scope_names() <= names
    assert len(in_scope_names()) == 44


def test_out_of_scope_codecs_are_unsupported(lib):
    scope = in_scope_names()
    out = [(i, nm) for i, nm in codec_names(lib).items() if nm not in scope]
    assert len(out) == CODEC_COUNT - 44
    for i, nm in out:
        assert enqueue(lib, i) == ERR_UNSUPPORTED, nm
        assert enqueue(lib, i, status=False) == ERR_UNSUPPORTED, nm      # (the codec set comes first)


def test_in_scope_codecs_fail_on_the_real_problem(lib):
    for i, nm in codec_names(lib).items():
        if nm not in in_scope_names():
            continue
        rc = enqueue(lib, i)
        assert rc in (ERR_DEVICE, ERR_CAPACITY), f"{nm}: {rc}"         # no GPU here / no workspace there
        assert enqueue(lib, i, status=False) == ERR_ARGUMENT, nm       # the status word is required
        assert enqueue(lib, i, n=0) == ERR_ARGUMENT, nm


def test_codec_ids_out_of_range(lib):
    assert enqueue(lib, -1) == ERR_ARGUMENT
    assert enqueue(lib, CODEC_COUNT) == ERR_ARGUMENT
