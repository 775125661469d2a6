"""Every outcome of the container encode rule (csrc/hsrle_codecs.h: encode_choice) on the GPU, one codec each, and the decode entry points' prologue.

Encode: containers of 64 full blocks and one partial block that ends off a 16-byte boundary, compressed three ways -- with the library's own scratch (every
split region), with a caller's workspace of hsrle_compress_workspace_size_codec (the regions the codec's path needs) and with one of
hsrle_compress_workspace_size (no regions for blocks of 1 .. 4 KiB); the callers' workspaces start 4 bytes off their allocation, so the size table is not
16-byte aligned and the scan takes its general form instead of the one-launch form.  Every container must be, byte for byte, the one
hsrle_testlib.build_container makes from the CPU oracle's block streams.  hsrle_encode_path speaks for the workspace without the small-block regions: its answer
is asserted for every case.

The first nine cases are a fixed list.  Four of its rows name a codec whose row of the launch table sends it elsewhere than the row's label says (rle8_7symlut and
rle32_3symlut_sym are position-parallel codecs: the former never reaches the split, run list or ring encoders in one piece, the latter's windowed launcher is the S
one); they stay, labelled with what the rule answers, and the four cases behind them reach those outcomes with rle8_7symlut_short and rle32_7symlut_sym.

Decode: the argument errors in their order of precedence through the three shipped entry points, against the status codes the library returned before the four
copies of the prologue became one (tests/golden/decode_prologue_status.json).  None of the calls launches anything."""
import ctypes
import json
import os
import random

import pytest

from hsrle_testlib import CODECS, CODEC_BY_KEY, build_container, fuzz_sections, mixed_runs, single_symbol_mix

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_prologue_status.json")
RING, SPLIT, RUN_LIST, PP = 0, 1, 2, 3          # include/hsrle.h: HSRLE_PATH_*
# (what the rule answers, codec, block size, hsrle_encode_path's answer)
CASES = [
    ("position-parallel", "rle8_packed_multi", 4096, PP),
    ("windowed, 8", "rle8_packed_multi", 8192, PP),
    ("windowed, S", "rle32_3symlut_sym", 8192, PP),
    ("windowed, S", "rle16_sym_short", 8192, PP),
    ("windowed, L", "rle8_7symlut", 8192, PP),
    ("split, lane chunks", "rle8_single", 8192, SPLIT),
    ("position-parallel", "rle8_7symlut", 4096, PP),
    ("position-parallel", "rle8_7symlut", 512, PP),
    ("small-block split", "rle16_1symlut_byte_short_greedy", 4096, RING),     # (split with the small-block regions, ring without: the answer is the latter's)
    ("windowed, L", "rle32_7symlut_sym", 8192, PP),
    ("split, list rounds", "rle8_7symlut_short", 8192, SPLIT),
    ("run list", "rle8_7symlut_short", 4096, RUN_LIST),
    ("ring", "rle8_7symlut_short", 512, RING),
]
TAIL = 267                                      # bytes of the last block (less than the smallest block size here): 11 past a 16-byte boundary


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    return hsrle


_DATA = {}


def _data(block):
    """64 blocks + TAIL bytes: runs of every symbol width, stretches of one favourite byte, random sections; made once per block size"""
    if block not in _DATA:
        rng, size = random.Random(1200 + block), 64 * block + TAIL
        parts, n = [], 0
        while n < size:
            k = rng.randrange(3)
            d = fuzz_sections(rng) if k == 0 else mixed_runs(rng, rng.choice([100, 1000, 3000])) if k == 1 else single_symbol_mix(rng, rng.choice([64, 333, 3000]))
            parts.append(d)
            n += len(d)
        _DATA[block] = b"".join(parts)[:size]
    return _DATA[block]


@pytest.mark.parametrize("outcome,key,block,path", CASES, ids=[f"{c[1]}-{c[2]}" for c in CASES])
def test_every_workspace_gives_the_oracles_container(hs, oracle, outcome, key, block, path):
    import numpy as np
    import torch

    codec, data = CODEC_BY_KEY[key], _data(block)
    cid = CODECS.index(codec)
    assert hs.codec_id(key) == cid
    assert hs.encode_path(key, len(data), block) == path, outcome
    expect = build_container(cid, len(data), block, oracle.compress_blocks(codec, np.frombuffer(data, dtype=np.uint8), block))
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()

    container, info = hs.compress(key, src, block_size=block)                      # the library's own scratch
    assert info.blockCount == 65 and container.cpu().numpy().tobytes() == expect, f"{key} {block}: own scratch ({outcome})"
    sizes = {"codec": hs.workspace_size(len(data), block, codec=key), "generic": hs.workspace_size(len(data), block)}
    assert sizes["codec"] > 0 and sizes["generic"] > 0
    if outcome == "small-block split":
        assert sizes["codec"] > 2 * len(data) > sizes["generic"]                   # the regions of the split encode: only the codec's size has them
    for which, n in sizes.items():
        ws = torch.full((n + 16,), 0xC3, dtype=torch.uint8, device="cuda")[4 : 4 + n]     # (garbage, and 4 bytes off: the size table is not 16-byte aligned)
        assert ws.data_ptr() % 16 == 4
        dst = torch.full((hs.container_bound(len(data), block),), 0x5A, dtype=torch.uint8, device="cuda")
        hs.compress_async(key, src, dst, block_size=block, workspace=ws)
        torch.cuda.synchronize()
        assert dst[: len(expect)].cpu().numpy().tobytes() == expect, f"{key} {block}: workspace of the {which} size ({outcome})"


# ---- the decode prologue ----
OK, ERR_ARGUMENT, ERR_CAPACITY, ERR_FORMAT = 0, 1, 2, 3
BLOCK, BLOCKS = 1024, 8
PACKET_LIST = 1          # include/hsrle.h: HSRLE_SPLIT_PACKET_LIST


def prologue_walk(L, info_type, container, out, stream=None):
    """{case: status} of the argument errors, each case with every LATER error present too, so that the status names the check that comes first.
    container / out: any two non-null device addresses -- no call gets as far as a launch."""
    U = BLOCK * (BLOCKS - 1) + 100

    def info(codec=1, block=BLOCK, count=BLOCKS):
        return info_type(version=1, codec=codec, uncompressedSize=U, blockSize=block, blockCount=count, payloadSize=U, totalSize=64 + 8 * (count + 1) + U + 32)

    entries = {
        "blocks": lambda c, i, first, count, o, cap: L.hsrle_decompress_blocks_dev_async(c, i, first, count, o, cap, None, stream),
        "whole": lambda c, i, first, count, o, cap: L.hsrle_decompress_dev_async(c, i, o, cap, None, stream),
        "split_none": lambda c, i, first, count, o, cap: L.hsrle_decompress_split_dev_async(c, i, first, count, o, cap, None, None, 0, BLOCK, stream),          # sub-block = block: the plain decode
        "split_list": lambda c, i, first, count, o, cap: L.hsrle_decompress_split_dev_async(c, i, first, count, o, cap, None, None, 0, PACKET_LIST, stream),
    }
    bad_infos = {"codec_id": info(codec=110), "block_size": info(block=1000), "block_count": info(count=BLOCKS + 1)}
    got = {}
    for name, call in entries.items():
        ref = lambda i: ctypes.byref(i) if i is not None else None
        # a null pointer beats a bad codec id (and everything behind it)
        got[f"{name}/null_container"] = call(None, ref(bad_infos["codec_id"]), BLOCKS, 5, out, 0)
        got[f"{name}/null_info"] = call(container, None, BLOCKS, 5, out, 0)
        got[f"{name}/null_out"] = call(container, ref(bad_infos["codec_id"]), BLOCKS, 5, None, 0)
        # a bad info beats a bad range and a short output
        for what, bad in bad_infos.items():
            got[f"{name}/bad_{what}"] = call(container, ref(bad), BLOCKS, 5, out, 0)
        # a bad range beats a short output ("whole" has no range: it answers for the capacity)
        good = info()
        got[f"{name}/range_past_the_end"] = call(container, ref(good), BLOCKS - 1, 2, out, 0)
        got[f"{name}/range_wraps_32_bits"] = call(container, ref(good), 0xFFFFFFFF, 2, out, 0)
        got[f"{name}/short_output"] = call(container, ref(good), 0, BLOCKS, out, U - 1)
        # nothing to do is not an error -- once everything in front of it, the device included, is in order ("whole" and the packet list go on to their own checks:
        # a workspace the split decode does not have)
        if name in ("blocks", "split_none"):
            got[f"{name}/no_blocks"] = call(container, ref(good), BLOCKS, 0, out, U)
        if name == "split_list":
            got[f"{name}/no_blocks"] = call(container, ref(good), BLOCKS, 0, out, U)
            got[f"{name}/no_workspace"] = call(container, ref(good), 0, BLOCKS, out, U)
    return got


def test_decode_prologue_order_and_status_codes(hs):
    import torch

    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    got = prologue_walk(hs.lib(), hs.ContainerInfo, ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf.data_ptr() + 32))
    with open(GOLDEN) as f:
        want = json.load(f)["status"]
    assert sorted(got) == sorted(want)
    for case, status in want.items():
        assert got[case] == status, case
    # the order the recorded codes stand for, said here too
    for name in ("blocks", "whole", "split_none", "split_list"):
        assert all(got[f"{name}/{c}"] == ERR_ARGUMENT for c in ("null_container", "null_info", "null_out")), name
        assert all(got[f"{name}/bad_{c}"] == ERR_FORMAT for c in ("codec_id", "block_size", "block_count")), name
        assert got[f"{name}/short_output"] == ERR_CAPACITY, name
        if name != "whole":
            assert got[f"{name}/range_past_the_end"] == got[f"{name}/range_wraps_32_bits"] == ERR_ARGUMENT and got[f"{name}/no_blocks"] == OK, name
    assert got["split_list/no_workspace"] == ERR_CAPACITY
