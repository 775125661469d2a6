"""The GPU decoders of the low-entropy family (csrc/hsrle_rle8m.hip.h) on streams written from the grammar (tests/low_entropy_grammar.py), against the
sequential model's bytes, exactly: the unsectioned stream through the drop-in names and hsrle_low_entropy_decompress_dev (piece and window edges,
the parity scan's limit and the one-wave fallback behind it, the store ladder, every header form), rle8m through the wave kernel (1 / 2 / 3 / 64
sections) and the lane kernel (131 072 sections), and one malformed stream per refusal rule of the parser.

Streams sit at even and at odd device addresses; outputs are filled with 0xEE and have 4 KiB guards on both sides; workspaces start as 0xC3.
tests/test_low_entropy_grammar.py holds the same fixtures against the oracle and the compiled reference on the CPU."""
import functools
import os
import struct

import numpy as np
import pytest

import low_entropy_grammar as G

pytestmark = pytest.mark.gpu

GUARD = 4096
LE_DROPINS = ("rle8_low_entropy_decompress", "rle8_low_entropy_short_decompress")
RLE8M_DROPINS = ("rle8m_decompress", "rle8m_opencl_decompress")
LE_COMPRESS = ("rle8_low_entropy_compress", "rle8_low_entropy_short_compress", "rle8_low_entropy_compress_only_max_frequency", "rle8_low_entropy_short_compress_only_max_frequency")


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    # (the A/B knob of csrc/hsrle_capi_low_entropy.h would send every rle8m stream to one kernel: the wave and lane tests below rely on the dispatch)
    assert "HSRLE_RLE8M_DECODE" not in os.environ, "HSRLE_RLE8M_DECODE overrides the rle8m kernel dispatch"
    import hsrle

    hsrle.lib()
    return hsrle


@functools.lru_cache(maxsize=None)
def le_want(name):
    return G.model(G.le_fixtures()[name], False)


@functools.lru_cache(maxsize=None)
def rle8m_want(name):
    return G.model(G.rle8m_fixtures()[name], True)


def to_dev(data, offset=0):
    import torch

    t = torch.zeros(len(data) + offset + 64, dtype=torch.uint8, device="cuda")[offset : offset + len(data)]
    t.copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))
    return t


def guarded(n, offset=0):
    """(the whole buffer, the n output bytes in it behind GUARD + offset bytes), all 0xEE"""
    import torch

    lead = GUARD + offset
    full = torch.full((lead + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    return full, full[lead : lead + n]


def read_back(full, n, offset=0):
    """(the n output bytes, both guards intact?)"""
    host = full.cpu().numpy()
    lead = GUARD + offset
    return host[lead : lead + n].tobytes(), bool((host[:lead] == 0xEE).all() and (host[lead + n :] == 0xEE).all())


def le_dev(hs, stream, n_out, offset=0):
    """hsrle_low_entropy_decompress_dev: (status code, size, output bytes, guards intact?, decode attempts)"""
    import torch

    src = to_dev(stream, offset)
    full, dst = guarded(n_out, offset)
    ws = torch.full((hs.low_entropy_decompress_workspace_size(len(stream)),), 0xC3, dtype=torch.uint8, device="cuda")
    rc, size = hs.low_entropy_decompress_dev(src, dst, ws)
    torch.cuda.synchronize()
    out, clean = read_back(full, n_out, offset)
    return rc, size, out, clean, hs.low_entropy_decode_attempts(ws)


def rle8m_dev(hs, stream, info=None, offset=0):
    """hsrle_rle8m_decompress_dev_async: (status word, output bytes, guards intact?)"""
    import torch

    src = to_dev(stream, offset)
    info = info or hs.rle8m_info(src)
    n_out = info.uncompressedSize
    full, dst = guarded(n_out, offset)
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hs.rle8m_decompress_async(src, info, dst, status)
    torch.cuda.synchronize()
    out, clean = read_back(full, n_out, offset)
    return int(status.item()), out, clean


def check_le(hs, name, stream, want, attempts=None):
    for offset in (0, 1, 3):
        rc, size, out, clean, tries = le_dev(hs, stream, len(want), offset)
        assert (rc, size) == (hs.OK, len(want)), f"{name} at offset {offset}"
        assert out == want, f"{name} at offset {offset}: decode differs from the model"
        assert clean, f"{name} at offset {offset}: wrote outside the output"
        if attempts is not None:
            assert tries == attempts, f"{name}: {tries} decode attempts"
    for fname in LE_DROPINS:
        assert hs.call_dropin(fname, stream, len(want)) == (len(want), want), f"{name}: {fname}"


def check_rle8m(hs, name, stream, want, offsets=(0, 1, 3), dropins=RLE8M_DROPINS):
    for offset in offsets:
        status, out, clean = rle8m_dev(hs, stream, None, offset)
        assert status == 0, f"{name} at offset {offset}"
        assert out == want, f"{name} at offset {offset}: decode differs from the model"
        assert clean, f"{name} at offset {offset}: wrote outside the output"
    for fname in dropins:
        assert hs.call_dropin(fname, stream, len(want)) == (len(want), want), f"{name}: {fname}"


# ------------------------------------------------------------------------------------------------------------------
# the unsectioned stream


@pytest.mark.parametrize("name", list(G.le_fixtures()))
def test_unsectioned(hs, name):
    """body sizes around the window and the piece, every placement at piece and window edges, whole flagged windows, the store ladder, every
    header form (a symbol listed twice: the last listing wins, as in the model)"""
    check_le(hs, name, G.le_fixtures()[name], le_want(name), attempts=1)


@pytest.mark.parametrize("name", list(G.le_limit_fixtures()))
def test_unsectioned_parity_scan_limit(hs, name):
    """65 535 flagged-valued bytes in front of a piece: one attempt; 65 536 and more, and a stream that is one such stretch: the scan gives up and
    the one-wave fallback gives the same bytes (the attempts: word 2 of the workspace, include/hsrle.h)"""
    stream, attempts = G.le_limit_fixtures()[name]
    check_le(hs, name, stream, G.model(stream, False), attempts=attempts)


def test_all_256_symbols_flagged_round_trip(hs, oracle):
    """the input on which every encoder flags all 256 symbols (the reference does not decode its own stream of it, include/hsrle.h): the four
    GPU encoders write the oracle's streams, both decoders give the input back; so does rle8m with 2 sections"""
    data = G.ALL_256_INPUT
    cap = len(data) + 1024
    for variant, cname in ((0, LE_COMPRESS[0]), (1, LE_COMPRESS[1]), (2, LE_COMPRESS[2]), (3, LE_COMPRESS[3])):
        size, stream = hs.call_dropin(cname, data, cap)
        assert size and stream == oracle.low_entropy_compress(variant, data), cname
        if variant < 2:
            assert G.parse(stream, False)[1]["flags.256"] == 1
        check_le(hs, cname, stream, data)
    stream = hs.rle8m_compress_dropin(2, data)
    assert stream == oracle.rle8m_compress(2, data) and G.parse(stream, True)[1]["flags.256"] == 1
    check_rle8m(hs, "rle8m_compress", stream, data)


# ------------------------------------------------------------------------------------------------------------------
# rle8m


@pytest.mark.parametrize("name", list(G.rle8m_fixtures()))
def test_rle8m_wave_kernel(hs, name):
    """the edge placements from each section's start with 1 / 2 / 3 / 64 sections; sections that end mid-window, on a window multiple, or hold
    nothing (uncompressedSize < sections); every header form"""
    stream = G.rle8m_fixtures()[name]
    assert struct.unpack_from("<I", stream, 8)[0] < 131072              # (the dispatch of csrc/hsrle_capi_low_entropy.h: a wave per section)
    check_rle8m(hs, name, stream, rle8m_want(name))


def test_rle8m_lane_kernel(hs):
    """131 072 sections of 300 bytes: the dispatch takes one lane per section.  64 patterns tiled: runs that enter the 16-byte accumulator at every
    phase with counts 0, 1, 15, 16, 17, 31, 32, 33, 254; a section of 100 tokens (the ring is topped up every 32 trips); a section without a flag"""
    stream, want = G.lane_stream()
    _, out_size, sections = struct.unpack_from("<III", stream, 0)
    assert sections >= 131072 and out_size // sections < 4096
    check_rle8m(hs, "lane", stream, want)


# ------------------------------------------------------------------------------------------------------------------
# malformed streams: refused by the kernels' bounds checks, nothing written outside the output


@pytest.mark.parametrize("name", list(G.le_malformed()))
def test_malformed_unsectioned_is_refused(hs, name):
    """HSRLE_ERR_FORMAT from the device entry point, 0 from the drop-in names, both guards intact.  What the output buffer itself holds behind a
    refused stream include/hsrle.h leaves open (the write pass is gated on the dry pass's total, but that is not a promise), so it is not asserted."""
    stream, _ = G.le_malformed()[name]
    n_out = struct.unpack_from("<I", stream, 4)[0]
    for offset in (0, 1):
        rc, size, _, clean, _ = le_dev(hs, stream, n_out, offset)
        assert rc == hs.ERR_FORMAT and size == 0, f"{name} at offset {offset}: status {rc}"
        assert clean, f"{name} at offset {offset}: wrote outside the output"
    for fname in LE_DROPINS:
        assert hs.call_dropin(fname, stream, n_out + 64) == (0, b""), f"{name}: {fname}"


@pytest.mark.parametrize("name", list(G.rle8m_malformed()))
def test_malformed_rle8m_is_refused(hs, name):
    """a nonzero status word from hsrle_rle8m_decompress_dev_async (the caller's info says what the caller can know: the buffer's size, the sizes
    the output was laid out for), HSRLE_ERR_FORMAT from hsrle_rle8m_info_dev where the three header words give it away, 0 from the drop-in names,
    both guards intact.  include/hsrle.h promises nothing about the sections of a refused stream, so their bytes are not asserted."""
    stream, rule = G.rle8m_malformed()[name]
    _, n_out, sections = struct.unpack_from("<III", stream, 0)
    if rule in ("size.above_buffer", "sections.zero", "info.past_stream"):
        with pytest.raises(hs.HsrleError) as e:
            hs.rle8m_info(to_dev(stream))
        assert e.value.status == hs.ERR_FORMAT
    for offset in (0, 1):
        info = hs.Rle8mInfo(len(stream), n_out, sections or 4)
        status, _, clean = rle8m_dev(hs, stream, info, offset)
        assert status != 0, f"{name} at offset {offset}"
        assert clean, f"{name} at offset {offset}: wrote outside the output"
    for fname in RLE8M_DROPINS:
        assert hs.call_dropin(fname, stream, n_out + 64) == (0, b""), f"{name}: {fname}"
