"""The encoders' 20-bit range rule on the GPU.  The LUT, Short and Greedy encoders and rle8_single_short store a run only if it pays for its header, and
the reference steps that penalty at 20 bits: a range or a stored count above 0xFFFFF costs 4, not 2 (src/rleX_Xsl.h:130, src/rleX_Xsl_short.h:197).
Only inputs with more than 1 MiB of literals in front of a run get there: the probes of tests/twenty_bit_probes.py, whose decisions
tests/golden/twenty_bit_probes.json records from the compiled reference (tests/test_twenty_bit_probes.py holds the oracle to them).

  * monolithic streams of all 82 codecs (drop-in, hsrle_compress_mono_dev, and hsrle_compress_mono_dev_enqueue where it takes the codec):
    the oracle's stream, and back through both decoders;
  * containers of blocks of 1 MiB + 1 KiB, one probe per block: the ring encoders (the windowed ones stop at kPpwListMaxBlock = 1 MiB - 128,
    below which no range reaches 0xFFFFF + 1);
  * containers of blocks of exactly 1 MiB: the one block size at which the split encode settles the lists of 2 .. 8 byte symbols inside
    k_encodeS_blocks."""
import numpy as np
import pytest

import twenty_bit_probes as P
from hsrle_testlib import CODEC_BY_KEY
from test_gpu_pp import WINDOWED_L_KEYS, WINDOWED_S_KEYS, _periodic

pytestmark = pytest.mark.gpu

KEYS = [c.key for c in P.RULE_CODECS]
PATH_RING, PATH_SPLIT, PATH_POSITION_PARALLEL = 0, 1, 3


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    return hsrle


@pytest.fixture(scope="module")
def golden():
    return P.load_golden()


def _mono(oracle, golden, key):
    """(codec, input, the oracle's stream) of one codec's monolithic input"""
    codec, g = CODEC_BY_KEY[key], golden["codecs"][key]["mono"]
    data, used = P.mono_input(codec, P.plan(codec, golden))
    want = oracle.compress(codec, data.tobytes())
    assert used == g["probes"] and (len(want), P.sha(want)) == (g["length"], g["sha256"]), f"{key}: the oracle's stream is not the golden file's"
    return codec, data, want


@pytest.mark.parametrize("key", KEYS)
def test_monolithic_stream_drop_in(hs, oracle, golden, key):
    """<codec>_compress and <codec>_decompress of rle.h (host pointers)."""
    codec, data, want = _mono(oracle, golden, key)
    raw = data.tobytes()
    size, stream = hs.call_dropin(codec.cname, raw, hs.compress_bounds(data.size))
    assert size == len(want) and stream == want, f"{key}: {codec.cname} differs from the oracle ({size} bytes, oracle {len(want)})"
    size, back = hs.call_dropin(codec.dname, want, data.size)
    assert size == data.size and back == raw, f"{key}: {codec.dname}"


@pytest.mark.parametrize("key", KEYS)
def test_monolithic_stream_device(hs, oracle, golden, key):
    """hsrle_compress_mono_dev, hsrle_compress_mono_dev_enqueue (where it takes the codec) and hsrle_decompress_mono_dev."""
    import torch

    codec, data, want = _mono(oracle, golden, key)
    n = data.size
    src = torch.from_numpy(data).cuda()
    got = hs.mono_compress_dev(key, src)
    assert got.cpu().numpy().tobytes() == want, f"{key}: hsrle_compress_mono_dev differs from the oracle ({got.numel()} bytes, oracle {len(want)})"

    if P.is_chunk_mode_short(codec):                                     # what hsrle_compress_mono_dev_enqueue accepts of these 82
        dst = torch.full((hs.compress_bounds(n) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        ws = hs._scratch(max(hs.mono_compress_workspace_size(key, n), 256), src.device)
        status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        word = torch.full((1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
        hs.mono_compress_dev_enqueue(key, src, dst, ws, status, word)
        torch.cuda.synchronize()
        assert int(status.item()) == hs.MONO_DONE, f"{key}: enqueue status {int(status.item())}"
        assert int(word.item()) == len(want), f"{key}: enqueue size word {int(word.item())}, oracle {len(want)}"
        assert dst[: len(want)].cpu().numpy().tobytes() == want, f"{key}: hsrle_compress_mono_dev_enqueue differs from the oracle"

    out = hs.mono_decompress_dev(key, got)
    assert out.numel() == n and torch.equal(out, src), f"{key}: hsrle_decompress_mono_dev"


def _check_container(hs, oracle, key, data, block):
    import torch

    codec = CODEC_BY_KEY[key]
    src = torch.from_numpy(data).cuda()
    container, _ = hs.compress(key, src, block_size=block)
    _, streams = hs.split_container(container.cpu().numpy().tobytes())
    expect = oracle.compress_blocks(codec, data, block)
    assert len(streams) == len(expect)
    bad = [i for i, (a, b) in enumerate(zip(streams, expect)) if a != b]
    assert not bad, f"{key} block size {block}: block streams {bad} of {len(expect)} differ from the oracle"
    assert torch.equal(hs.decompress(container), src), f"{key} block size {block}: decode"
    return expect


@pytest.mark.parametrize("key", KEYS)
def test_container_blocks_above_one_mib(hs, oracle, golden, key):
    codec, g = CODEC_BY_KEY[key], golden["codecs"][key]["container"]
    data = P.container_input(codec, P.plan(codec, golden))
    assert hs.encode_path(key, data.size, P.BLOCK) == PATH_RING
    if key in WINDOWED_L_KEYS or key in WINDOWED_S_KEYS:                   # the control: the largest block no range T + 1 fits in stays position-parallel
        assert hs.encode_path(key, data.size, (1 << 20) - 128) == PATH_POSITION_PARALLEL
    expect = _check_container(hs, oracle, key, data, P.BLOCK)
    assert [len(s) for s in expect] == g["lengths"] and P.sha(b"".join(expect)) == g["sha256"], f"{key}: the oracle's streams are not the golden file's"


def test_the_control_covers_the_windowed_codecs():
    assert len([k for k in KEYS if k in WINDOWED_L_KEYS or k in WINDOWED_S_KEYS]) == 64


ONE_MIB_KEYS = ["rle16_3symlut_byte", "rle24_7symlut_sym", "rle32_3symlut_sym", "rle64_7symlut_byte", "rle16_7symlut_sym_short", "rle48_3symlut_byte_short",   # lists in the kernel
                "rle8_3symlut", "rle8_7symlut_short",                                                                                                         # lists between launches
                "rle32_1symlut_byte_short_greedy", "rle128_sym_packed"]                                                                                       # lane chunks

_one_mib_inputs = {}


def _one_mib_input(S):
    """Three blocks of 1 MiB and a ragged fourth: periodic stretches of a 5-letter alphabet (period 1: five symbols that every list comes to hold; period S:
    others) with literal gaps of at most 40 bytes, lengths around every store threshold -- and in the second block a run of 600 000 bytes."""
    if S not in _one_mib_inputs:
        rng = np.random.default_rng(1 << 20 | S)
        B, n = 1 << 20, 3 * (1 << 20) + 300001
        lengths = sorted({S + 1, 2 * S, 2 * S + 1, 3 * S, 3 * S + 2, 4 * S + 1, S + 10, S + 11, S + 12, S + 13, 40, 64, 300})
        data = _periodic(rng, n, [1, S, S], 5, 40, lengths)
        data[B + 100000 : B + 700000] = np.tile(rng.integers(0, 5, S, dtype=np.uint8), 600000 // S + 1)[:600000]
        _one_mib_inputs[S] = data                                          # (shared: nobody writes to it)
    return _one_mib_inputs[S]


@pytest.mark.parametrize("key", ONE_MIB_KEYS)
def test_container_blocks_of_one_mib(hs, oracle, key):
    data = _one_mib_input(CODEC_BY_KEY[key].S)
    assert hs.encode_path(key, data.size, 1 << 20) == PATH_SPLIT
    _check_container(hs, oracle, key, data, 1 << 20)
