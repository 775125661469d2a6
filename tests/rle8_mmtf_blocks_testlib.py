"""Helpers of the rle8_mmtf128 block container tests (include/hsrle.h section 5): the container built, split and decoded in plain Python.  Block stream i
is this library's rle8_mmtf128 stream of input bytes [i B, min((i + 1) B, n)): rle8_mmtf_testlib.model_compress, held against the compiled reference by
test_rle8_mmtf_model.py -- the move-to-front lists are the identity at the start of every block, the first packet's start value is zero.

  [ 0] "HSRLEMFB"  [ 8] u32 version = 1  [12] u32 reserved = 0  [16] u64 uncompressedSize  [24] u32 blockSize  [28] u32 blockCount
  [32] u64 payloadSize  [40] u64 totalSize = 64 + 8 * (blockCount + 1) + payloadSize + 32  [48] 16 zero bytes
  [64] u64 offset[blockCount + 1], relative to the payload; the block streams back to back; 32 zero bytes
"""
import struct

import rle8_mmtf_testlib as T

MAGIC = b"HSRLEMFB"
HEADER, PAD = 64, 32
DEFAULT_BLOCK = 4096
STREAM_SLACK = 13                # inSize + 13 always suffices for one stream (include/hsrle.h)
_STREAMS = {}


def valid_block_size(B):
    return 128 <= B <= 1 << 20 and B % 128 == 0


def block_count(n, B):
    return (n + B - 1) // B


def bound(n, B):
    B = B or DEFAULT_BLOCK
    if n == 0 or not valid_block_size(B) or block_count(n, B) >= 1 << 32:
        return 0
    nb = block_count(n, B)
    return HEADER + 8 * (nb + 1) + n + STREAM_SLACK * nb + PAD


def blocks_of(data, B):
    return [data[i : i + B] for i in range(0, len(data), B)]


def block_stream(block):
    """model_compress, remembered: the tests share blocks."""
    block = bytes(block)
    if block not in _STREAMS:
        _STREAMS[block] = T.model_compress(block)
    return _STREAMS[block]


def from_streams(streams, n, B, offsets=None):
    """The container of given block streams (nothing is checked: malformed ones can be built); offsets: a table to write instead of the true one."""
    payload = b"".join(streams)
    if offsets is None:
        offsets, at = [0], 0
        for s in streams:
            at += len(s)
            offsets.append(at)
    nb = len(streams)
    total = HEADER + 8 * (nb + 1) + len(payload) + PAD
    head = MAGIC + struct.pack("<IIQIIQQ", 1, 0, n, B, nb, len(payload), total) + bytes(16)
    assert len(head) == HEADER
    return head + struct.pack(f"<{nb + 1}Q", *offsets) + payload + bytes(PAD)


def build(data, B):
    data = bytes(data)
    return from_streams([block_stream(b) for b in blocks_of(data, B)], len(data), B)


def header(container):
    version, reserved, n, B, nb, payload, total = struct.unpack_from("<IIQIIQQ", container, 8)
    return {"magic": bytes(container[:8]), "version": version, "reserved": reserved, "uncompressedSize": n, "blockSize": B, "blockCount": nb, "payloadSize": payload,
            "totalSize": total, "zero": bytes(container[48:64])}


def split(container):
    """(header fields, [block stream bytes]) of a well-formed container; asserts every relation of the format."""
    container = bytes(container)
    h = header(container)
    nb = h["blockCount"]
    assert h["magic"] == MAGIC and h["version"] == 1 and h["reserved"] == 0 and h["zero"] == bytes(16)
    assert valid_block_size(h["blockSize"]) and nb == block_count(h["uncompressedSize"], h["blockSize"])
    start = HEADER + 8 * (nb + 1)
    assert h["totalSize"] == start + h["payloadSize"] + PAD == len(container)
    off = struct.unpack_from(f"<{nb + 1}Q", container, HEADER)
    assert off[0] == 0 and off[nb] == h["payloadSize"] and all(a <= b for a, b in zip(off, off[1:]))
    assert container[start + h["payloadSize"] :] == bytes(PAD)
    return h, [container[start + off[i] : start + off[i + 1]] for i in range(nb)]


def decode(container):
    """The bytes of a well-formed container through the model decoder, or None if any block is malformed."""
    h, streams = split(container)
    out = bytearray()
    for i, s in enumerate(streams):
        back = T.model_decompress(s)
        want = min(h["blockSize"], h["uncompressedSize"] - i * h["blockSize"])
        if back is None or len(back) != want:
            return None
        out += back
    return bytes(out)


def data_from_block_specs(specs, B, tail=b"", seed=1):
    """The input whose block i has exactly the packets of specs[i] (rle8_mmtf_testlib.rows_from_spec: ("rle", count, rank) / ("copy", count, top rank)):
    the blocks are independent -- identity lists at every block start --, so each block's bytes are the inverse mmtf of its own rank rows.  Every block
    but the last must fill its B / 16 rows; `tail`: the tail ranks of the last block."""
    out = bytearray()
    for i, spec in enumerate(specs):
        rows = T.rows_from_spec(spec, seed + i)
        last = i == len(specs) - 1
        assert len(rows) == B // 16 or (last and len(rows) <= B // 16), (i, len(rows))
        out += T.data_from_rank_rows(rows, tail if last else b"")
    return bytes(out)
