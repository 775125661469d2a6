"""Windowed encoders (csrc/hsrle_encode8pw.hip.h, hsrle_encodeSpw.hip.h, hsrle_encodeLpw.hip.h), block mode: a container's LAST block that ends -1 .. S + 1 bytes
behind a 4 KiB window edge -- on a run that reaches its end (the window in FRONT of the last one stores that run where the block ends 1 .. S - 1 bytes into a
window, and the last window still has to write the "ended" terminator the scan pass sized), a few bytes short of the end (trailing literals that begin in front
of the last window), on literals only.  Inputs: tests/block_end_cases.py; what they are is checked without a GPU in tests/test_block_end_cases.py.
Every block stream == the oracle's, nothing is written behind the container, the reported size is the sum of the oracle's, and both readers of the terminator
(the block decode, the range decode) give the input back."""
import numpy as np
import pytest

import block_end_cases as BE
from hsrle_testlib import CODEC_BY_KEY

pytestmark = pytest.mark.gpu

GUARD = 0xA5


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()  # fails loudly if the HIP library is missing
    return hsrle


class Expect:
    """the oracle's block streams of a codec's cases: the two full blocks once per block size, the last block per case"""

    def __init__(self, oracle, codec):
        self.oracle, self.codec, self.front = oracle, codec, {}

    def streams(self, c):
        if c.B not in self.front:
            self.front[c.B] = self.oracle.compress_blocks(self.codec, c.data[: 2 * c.B], c.B)
        return self.front[c.B] + self.oracle.compress_blocks(self.codec, c.data[2 * c.B :], c.B)


def _verdict(hs, c, expect, dst, src):
    """None, or what is wrong with the container that compressing case `c` left in `dst` (a buffer of container_bound + 64 bytes that held GUARD everywhere)"""
    import torch

    host = dst.cpu().numpy()
    info = hs.container_info(host.tobytes())
    size = int(info.totalSize)
    _, streams = hs.split_container(host[:size].tobytes())
    if len(streams) != len(expect):
        return f"{len(streams)} blocks, not {len(expect)}"
    bad = [i for i, (a, b) in enumerate(zip(streams, expect)) if a != b]
    if bad:
        i = bad[-1]
        a, b = streams[i], expect[i]
        at = next((j for j in range(min(len(a), len(b))) if a[j] != b[j]), min(len(a), len(b)))
        return f"block stream(s) {bad} differ from the oracle's: block {i} has {len(a)} bytes (oracle {len(b)}), first difference at byte {at}: {a[at : at + 12].hex()} != {b[at : at + 12].hex()}"
    touched = np.flatnonzero(host[size:] != GUARD)
    if touched.size:
        return f"{touched.size} bytes behind the container's {size} were written, the first {int(touched[0])} and the last {int(touched[-1])} bytes behind its end"
    want = hs.HEADER_SIZE + 8 * (len(expect) + 1) + sum(len(s) for s in expect) + hs.TAIL_PAD
    if size != want:
        return f"the container says {size} bytes, header + offset table + the oracle's streams + pad are {want}"
    if not torch.equal(hs.decompress(dst[:size]), src):
        return "decode differs from the input"
    return None


def _report(key, bad, total):
    assert not bad, f"{key}: {len(bad)} of {total} cases fail -- {BE.summary([n for n, _ in bad])}\n" + "\n".join(f"  {key} {n}: {why}" for n, why in bad[:40])


@pytest.mark.parametrize("key", BE.ALL_KEYS)
def test_last_block_behind_a_window_edge(hs, oracle, key):
    import torch

    codec = CODEC_BY_KEY[key]
    expect = Expect(oracle, codec)
    bad, total = [], 0
    for c in BE.case_list(codec):
        total += 1
        src = torch.from_numpy(c.data).cuda()
        dst = torch.full((hs.container_bound(c.data.size, c.B) + 64,), GUARD, dtype=torch.uint8, device="cuda")
        container, _ = hs.compress(key, src, block_size=c.B, dst=dst)
        why = _verdict(hs, c, expect.streams(c), dst, src)
        if why is None and container.numel() != int(hs.container_info(container).totalSize):
            why = "hsrle_compress_dev's size is not the header's"
        if why:
            bad.append((c.name, why))
    _report(key, bad, total)


@pytest.mark.parametrize("key", BE.REPRESENTATIVE_KEYS)
def test_odd_source_addresses_and_dirty_memory(hs, oracle, key):
    """the same cases read from a source 1 .. 7 bytes into a larger tensor, compress_async with a caller's workspace full of garbage"""
    import torch

    codec = CODEC_BY_KEY[key]
    expect = Expect(oracle, codec)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(codec.S)
    bad, total = [], 0
    for c in BE.case_list(codec):
        U = c.data.size
        off = 1 + total % 7
        total += 1
        buf = torch.zeros(U + 16, dtype=torch.uint8, device="cuda")
        src = buf[off : off + U]
        src.copy_(torch.from_numpy(c.data))
        dst = torch.full((hs.container_bound(U, c.B) + 64,), GUARD, dtype=torch.uint8, device="cuda")
        ws = torch.randint(0, 256, (max(hs.workspace_size(U, c.B, key), 16),), dtype=torch.uint8, device="cuda", generator=gen)
        hs.compress_async(key, src, dst, block_size=c.B, workspace=ws)
        torch.cuda.synchronize()
        why = _verdict(hs, c, expect.streams(c), dst, src)
        if why:
            bad.append((c.name + f" offset {off}", why))
    _report(key, bad, total)


@pytest.mark.parametrize("key", BE.REPRESENTATIVE_KEYS)
def test_range_decode_reads_the_ended_terminator(hs, oracle, key):
    """hsrle_decompress_range_dev_async over the last S + 4096 bytes of every `to_end` container: the other reader of the last block's terminator"""
    import torch

    codec = CODEC_BY_KEY[key]
    n = codec.S + BE.WINDOW
    bad, total = [], 0
    for c in BE.case_list(codec):
        if c.shape != "to_end":
            continue
        total += 1
        U = c.data.size
        src = torch.from_numpy(c.data).cuda()
        container, info = hs.compress(key, src, block_size=c.B)
        out = torch.full((n + 64,), GUARD, dtype=torch.uint8, device="cuda")
        status = torch.full((4,), 0xFF, dtype=torch.uint8, device="cuda")
        hs.decompress_range_dev_async(container, info, U - n, n, out[:n], status)
        torch.cuda.synchronize()
        st = int.from_bytes(status.cpu().numpy().tobytes(), "little")
        got = out.cpu().numpy()
        if st != hs.MONO_DONE:
            bad.append((c.name, f"status {st}"))
        elif not np.array_equal(got[:n], c.data[U - n :]):
            bad.append((c.name, "the range differs from the input's bytes"))
        elif not (got[n:] == GUARD).all():
            bad.append((c.name, "bytes behind the range were written"))
    assert total == 2 * len(BE.BLOCKS_AND_WINDOWS) * len(BE.remainders(codec.S))
    _report(key, bad, total)
