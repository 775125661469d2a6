"""The host-pointer drop-in functions of all families stage through ONE set of per-device buffers (csrc/hsrle_capi_host.h: Staging): what no
other test does is to reuse them across families and across sizes in one process -- grow, shrink (the zero tail behind a shorter stream must be
written again: the bytes behind it are the longer stream's), the split-phase helpers in between, grow again.  Every stream is compared with the
oracle's bytes, every decode (of the oracle's stream) with the input.  The smaller inputs are the large one's bytes inverted: run-distributed too,
and different from what the buffers held at every offset.
The mmtf / bitmmtf transforms and rle8_mmtf128 stage through the same buffers: their calls stand between the others', at every size, and are compared with
the sequential models (tests/mmtf_testlib.py, tests/rle8_mmtf_testlib.py) -- a 100-byte call behind another family's 1 MiB call must not see its bytes."""
import ctypes
import struct

import pytest

import mmtf_testlib as M
import rle8_mmtf_testlib as R
import test_gpu_low_entropy_helpers as helpers
from hsrle_testlib import CODEC_BY_KEY

pytestmark = pytest.mark.gpu

SECTIONS = 7


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    return hsrle


def _six_calls(hs, oracle, data, below_bound=False):
    """low-entropy, rle8m (7 sections), 8 bit Packed: compress == the oracle's stream, decompress of it == data"""
    lib = hs.lib()
    n = len(data)
    packed = CODEC_BY_KEY["rle8_packed_multi"]
    cases = (("rle8_low_entropy_compress", "rle8_low_entropy_decompress", lib.rle8_low_entropy_compress_bounds(ctypes.c_uint32(n)), oracle.low_entropy_compress(0, data)),
             (None, "rle8m_decompress", hs.rle8m_bounds(SECTIONS, n), oracle.rle8m_compress(SECTIONS, data)),
             (packed.cname, packed.dname, hs.compress_bounds(n), oracle.compress(packed, data)))
    for cname, dname, cap, want in cases:
        assert want is not None, f"{dname}: the oracle has no stream for this input"
        if cname is None:
            got = hs.rle8m_compress_dropin(SECTIONS, data)
        else:
            size, got = hs.call_dropin(cname, data, cap)
            assert size == len(want), f"{cname} on {n} bytes"
        assert got == want, f"{cname or 'rle8m_compress'} on {n} bytes: stream differs from the oracle's"
        size, dec = hs.call_dropin(dname, want, n)
        assert size == n and dec == data, f"{dname} on {n} bytes"
        if below_bound:
            if cname is None:
                out = ctypes.create_string_buffer(cap)
                assert lib.rle8m_compress(ctypes.c_uint32(SECTIONS), data, ctypes.c_uint32(n), out, ctypes.c_uint32(cap - 1)) == 0
            else:
                assert hs.call_dropin(cname, data, cap - 1)[0] == 0
            assert hs.call_dropin(dname, want, n - 1)[0] == 0


_MODELS = {}


def _model(kind, data, make):
    """the sequential models are slow on 1 MiB: once per input"""
    if (kind, data) not in _MODELS:
        _MODELS[(kind, data)] = make(data)
    return _MODELS[(kind, data)]


def _mmtf_calls(hs, data, below_bound=False):
    """mmtf128, bitmmtf8, rle8_mmtf128: encode / compress == the model's bytes, decode / decompress of them == data"""
    n = len(data)
    for transform in (M.MMTF128, M.BITMMTF8):
        enc, dec = getattr(hs, M.function_name(transform, 0)), getattr(hs, M.function_name(transform, 1))
        want = _model(transform, data, lambda d: M.model(transform, 0, d))
        assert enc(data) == (n, want), f"{enc.__name__} on {n} bytes"
        assert dec(want) == (n, data), f"{dec.__name__} on {n} bytes"
        if below_bound:
            assert enc(data, n - 1)[0] == 0 and dec(want, n - 1)[0] == 0
    want = _model("rle8_mmtf128", data, R.model_compress)
    assert hs.rle8_mmtf128_compress(data) == (len(want), want), f"rle8_mmtf128_compress on {n} bytes: stream differs from the model's"
    assert hs.rle8_mmtf128_decompress(want, n) == (n, data), f"rle8_mmtf128_decompress on {n} bytes"
    if below_bound:
        assert hs.rle8_mmtf128_compress(data, out_cap=hs.rle8_mmtf128_compress_bounds(n) - 1)[0] == 0
        assert hs.rle8_mmtf128_decompress(want, n - 1)[0] == 0


def test_staging_buffers_reused_across_families_and_sizes(hs, oracle):
    hs.mmtf_tuning(0)
    hs.rle8_mmtf_tuning(0)
    big = oracle.synth(hs.SYNTH_RUNS, 1, 11, (1 << 20) + 3).tobytes()
    inverted = bytes(b ^ 0xFF for b in big[:4097])
    _six_calls(hs, oracle, big)
    _mmtf_calls(hs, big)
    for n in (4097, 100):
        _six_calls(hs, oracle, inverted[:n], below_bound=True)
        _mmtf_calls(hs, inverted[:n], below_bound=True)

    # the split-phase helpers on the same buffers: statistics, header, body == the oracle's whole stream; header reader + body decode == the input
    data = inverted
    lib = hs.lib()
    want = oracle.low_entropy_compress(0, data)
    info = helpers.CompressInfo()
    assert lib.rle8_low_entropy_get_compress_info(data, len(data), ctypes.byref(info))
    head = ctypes.create_string_buffer(600)
    hsize = lib.rle8_low_entropy_write_compress_info(ctypes.byref(info), head, 600)
    body = helpers._body(lib, "rle8_low_entropy_compress_with_info", data, info)
    assert body is not None
    assert struct.pack("<II", 8 + hsize + len(body), len(data)) + head.raw[:hsize] + body == want
    out = ctypes.create_string_buffer(len(data))
    assert lib.rle8_low_entropy_compress_with_info(data, len(data), ctypes.byref(info), out, len(data) - 1) == 0      # outSize below the input's size
    dinfo = helpers.DecompressInfo()
    assert lib.rle8_low_entropy_read_decompress_info(want[8:], len(want) - 8, ctypes.byref(dinfo)) == hsize
    assert helpers._decode(lib, "rle8_low_entropy_decompress_with_info", body, dinfo, len(data)) == data

    _mmtf_calls(hs, inverted[:100], below_bound=True)                  # (behind the helpers' calls)
    _six_calls(hs, oracle, big)                                        # ... and the buffers grow again
    _mmtf_calls(hs, big)
