"""The checkpoints and the byte-range decode of rle8_mmtf128 streams on the GPU (csrc/hsrle_rle8mmtf_range.hip.h) against their model
(tests/rle8_mmtf_range_testlib.py, held against the transform and the inputs by test_rle8_mmtf_range_model.py).  The built sidecar is the model's, byte for
byte, whatever the tuning knobs; a range decode gives data[offset : offset + length] with DONE and writes nothing outside dOut[0, length); sidecars that do
not go with the stream end in INDEX or CHECKPOINT with dOut untouched, and no bytes in either sidecar make the decode write anywhere else."""
import json
import struct

import numpy as np
import pytest

import rle8_mmtf_index_testlib as X
import rle8_mmtf_range_testlib as G
import rle8_mmtf_testlib as T

pytestmark = pytest.mark.gpu

GUARD = 4096
DONE, MALFORMED, CAPACITY, INDEX, CHECKPOINT = 0, 1, 2, 3, 4
STREAMS = G.range_streams()
_SIDE = {}


def model_side(data, ck_rows, stream_size):
    key = (data, ck_rows, stream_size)
    if key not in _SIDE:
        _SIDE[key] = G.model_checkpoints(data, ck_rows, stream_size)
    return _SIDE[key]


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    hsrle.mmtf_tuning(0)
    hsrle.rle8_mmtf_tuning(0)
    yield hsrle
    hsrle.mmtf_tuning(0)
    hsrle.rle8_mmtf_tuning(0)


@pytest.fixture
def tuned(hs):
    yield hs
    hs.mmtf_tuning(0)                                                        # (process-global)
    hs.rle8_mmtf_tuning(0)


def to_dev(data, offset=0, slack=64):
    import torch

    t = torch.zeros(len(data) + offset + slack, dtype=torch.uint8, device="cuda")[offset : offset + len(data)]
    t.copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))
    return t


def guarded(n, offset):
    """(whole buffer of 0xEE, the n bytes at `offset` of it)"""
    import torch

    full = torch.full((offset + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    return full, full[offset : offset + n]


def untouched(full, offset, n):
    host = full.cpu().numpy()
    return bool((host[:offset] == 0xEE).all() and (host[offset + n :] == 0xEE).all())


def garbage(n, offset):
    import torch

    return torch.full((n + offset,), 0xC3, dtype=torch.uint8, device="cuda")[offset:]


def build_dev(hs, stream, index, ck_rows, offsets=(0, 0, 0, 0), info=None):
    """(status, size word, sidecar bytes, the whole buffer's bytes, nothing written outside the sidecar?); offsets: stream, sidecar, workspace, index"""
    import torch

    info = hs.rle8_mmtf128_index_info(index) if info is None else info
    n = info.uncompressedSize
    cap = hs.rle8_mmtf128_checkpoints_bound(n, ck_rows)
    full, out = guarded(cap, offsets[1])
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    size = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    hs.rle8_mmtf128_checkpoints_build_dev(to_dev(stream, offsets[0]), to_dev(index, offsets[3]), info, out, size, status,
                                          garbage(hs.rle8_mmtf128_workspace_size(True, n), offsets[2]), checkpoint_rows=ck_rows)
    torch.cuda.synchronize()
    got = int(size.item())
    whole = out.cpu().numpy().tobytes()
    return int(status.item()), got, whole[:got], whole, untouched(full, offsets[1], cap)


class Ranges:
    """One stream and its two sidecars on the device, at odd addresses; every run gets a fresh output between guard bytes, at an odd address, and a workspace
    of exactly hsrle_rle8_mmtf128_range_workspace_size(length, ...) bytes of garbage.  info / ck: the headers the host holds (default: the sidecars' own)."""

    def __init__(self, hs, stream, index, side, offsets=(1, 3, 5, 7, 9), info=None, ck=None):
        self.hs = hs
        self.src, self.idx, self.side = to_dev(stream, offsets[0]), to_dev(index, offsets[3]), to_dev(side, offsets[4])
        self.info = hs.rle8_mmtf128_index_info(index) if info is None else info
        self.ck = hs.rle8_mmtf128_checkpoints_info(side) if ck is None else ck
        self.out_at, self.ws_at = offsets[1], offsets[2]

    def run(self, offset, length):
        """(status, dOut[0, length), the guard bytes around it intact?)"""
        import torch

        full, dst = guarded(length, self.out_at)
        status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        ws = garbage(self.hs.rle8_mmtf128_range_workspace_size(length, self.info.spacing, self.ck.checkpointRows), self.ws_at)
        self.hs.rle8_mmtf128_decompress_range_dev(self.src, self.idx, self.info, self.side, self.ck, offset, length, dst, status, ws)
        host = full.cpu().numpy()
        lo, hi = self.out_at, self.out_at + length
        return int(status.item()), host[lo:hi].tobytes(), bool((host[:lo] == 0xEE).all() and (host[hi:] == 0xEE).all())


# ---- build ----

@pytest.mark.parametrize("ck_rows", G.CHECKPOINT_ROWS)
def test_built_sidecar_is_the_models(hs, ck_rows):
    for name, data in X.encoder_inputs().items():
        stream = T.model_compress(data)
        want = model_side(data, ck_rows, len(stream))
        for offsets in ((0, 0, 0, 0), (3, 1, 7, 5)):
            status, size, side, _, clean = build_dev(hs, stream, X.model_index(stream, 64), ck_rows, offsets)
            assert (status, size, clean) == (DONE, len(want), True), name
            assert side == want, f"{name}: the built checkpoints differ from the model's"


def test_built_sidecar_of_a_reference_written_stream(hs):
    with open(T.GOLDEN) as f:
        v = {v["name"]: v for v in json.load(f)["vectors"]}["headers_32_128"]
    data, stream = bytes.fromhex(v["input"]), bytes.fromhex(v["stream"])
    assert len(data) // 16 > 4 * 64
    for ck_rows in G.CHECKPOINT_ROWS:
        want = model_side(data, ck_rows, len(stream))
        status, size, side, _, clean = build_dev(hs, stream, X.model_index(stream, 64), ck_rows)
        assert (status, size, side, clean) == (DONE, len(want), want, True), ck_rows


@pytest.fixture(scope="module")
def mixed():
    data = G.mixed_input()
    stream = T.model_compress(data)
    assert 2000 <= len(data) // 16 < 2300 and len(data) % 16 == 3
    return data, stream, X.model_index(stream, 64), model_side(data, 256, len(stream))


def test_tuning_knobs_do_not_change_the_sidecar(tuned, mixed):
    """segments of 16 and 64 rows divide a checkpoint row, 48 does not (rows are applied behind the segment's list), 256 is the checkpoint spacing itself"""
    data, stream, index, _ = mixed
    a, _ = X.tamper_base()
    small = T.model_decompress(a)
    for segment, span in ((16, 0), (48, 7), (64, 63), (256, 1), (0, 0)):
        tuned.mmtf_tuning(segment)
        tuned.rle8_mmtf_tuning(span)
        for ck_rows in (64, 128, 256):
            status, size, side, _, clean = build_dev(tuned, stream, index, ck_rows)
            assert (status, clean) == (DONE, True) and side == model_side(data, ck_rows, len(stream)), (segment, span, ck_rows)
        status, size, side, _, clean = build_dev(tuned, a, X.model_index(a, 64), 64, (1, 3, 5, 7))
        assert (status, clean) == (DONE, True) and side == model_side(small, 64, len(a)), (segment, span)


def test_build_writes_nothing_behind_malformed_and_index(hs):
    import torch

    for name, (n, stream) in X.malformed_streams().items():
        index = X.pack_index(n, max(struct.unpack_from("<I", stream, 4)[0], 10), 64, [])
        info = hs.rle8_mmtf128_index_info(index)
        status, size, _, whole, clean = build_dev(hs, stream, index, 64, info=info)
        # what decompress_indexed says of the same stream and index
        full, dst = guarded(n, 0)
        word = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        hs.rle8_mmtf128_decompress_indexed_dev(to_dev(stream), to_dev(index), info, dst, word, garbage(hs.rle8_mmtf128_workspace_size(True, n), 0))
        torch.cuda.synchronize()
        assert status == int(word.item()) and status in (MALFORMED, INDEX), name
        assert (size, clean) == (0, True) and G.MAGIC not in whole, name
    a, b = X.tamper_base()
    status, size, _, whole, clean = build_dev(hs, a, X.model_index(b, 64), 64)
    assert (status, size, clean) == (INDEX, 0, True) and G.MAGIC not in whole


# ---- range decode ----

@pytest.mark.parametrize("ck_rows", G.CHECKPOINT_ROWS)
def test_range_grid(hs, ck_rows):
    """the model test's grid of (stream, offset, length) against the input: odd addresses, guard bytes, a workspace of garbage at every call"""
    for name, (stream, data) in STREAMS.items():
        r = Ranges(hs, stream, X.model_index(stream, 64), model_side(data, ck_rows, len(stream)))
        for offset, length in G.range_grid(len(data)):
            status, got, clean = r.run(offset, length)
            assert (status, clean) == (DONE, True), f"{name} [{offset}, +{length})"
            assert got == data[offset : offset + length], f"{name} [{offset}, +{length})"


def test_ranges_across_checkpoints_and_segments(tuned, mixed):
    import torch

    data, stream, index, side = mixed
    n, rows = len(data), len(data) // 16
    ranges = {
        "across two checkpoints": (16 * 300 + 3, 16 * 700 + 9),              # from checkpoint 256 over 512 and 768
        "starts on a checkpoint row": (16 * 512, 1000),
        "ends on a checkpoint row": (16 * 520 + 7, 16 * 768 - (16 * 520 + 7)),
        "from the identity": (16 * 100 + 1, 16 * 100),                       # c = 0: no checkpoint is read
        "the last rows and the tail": (16 * (rows - 300) + 5, n - (16 * (rows - 300) + 5)),
        "the tail alone": (n - 2, 2),
        "the whole stream": (0, n),
    }
    for segment in (16, 64):
        tuned.mmtf_tuning(segment)
        r = Ranges(tuned, stream, index, side)
        for name, (offset, length) in ranges.items():
            status, got, clean = r.run(offset, length)
            assert (status, clean) == (DONE, True), (segment, name)
            assert got == data[offset : offset + length], (segment, name)
        # the whole stream's range is decompress_indexed's output
        full, dst = guarded(n, 0)
        word = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        tuned.rle8_mmtf128_decompress_indexed_dev(to_dev(stream), to_dev(index), r.info, dst, word, garbage(tuned.rle8_mmtf128_workspace_size(True, n), 0))
        torch.cuda.synchronize()
        assert int(word.item()) == DONE and dst.cpu().numpy().tobytes() == r.run(0, n)[1]
    # an index spacing above the checkpoint spacing: e0 lies far in front of row c
    tuned.mmtf_tuning(0)
    r = Ranges(tuned, stream, X.model_index(stream, 1024), model_side(data, 64, len(stream)))
    for offset, length in ((16 * 1000 + 3, 500), (16 * 1100, 16 * 300), (5, 16 * 70), (n - 40, 40)):
        assert r.run(offset, length) == (DONE, data[offset : offset + length], True), (offset, length)


@pytest.fixture(scope="module")
def base(hs):
    a, b = X.tamper_base()
    data = T.model_decompress(a)
    return a, b, data, X.model_index(a, 64), model_side(data, 64, len(a))


RANGE = (16 * 130 + 5, 16 * 100)                                             # rows 130 .. 230 of tamper_base: from checkpoint 2 (row 128), entries of rows 70 .. 290


def test_checkpoint_tampers(hs, base):
    a, _, data, index, side = base
    offset, length = RANGE
    want = data[offset : offset + length]
    info, ck = hs.rle8_mmtf128_index_info(index), hs.rle8_mmtf128_checkpoints_info(side)
    assert Ranges(hs, a, index, side).run(offset, length) == (DONE, want, True)
    used, other = 64 + 4096 * (128 // 64 - 1), 64 + 4096 * 4
    for col in (0, 3, 15):
        at = used + 256 * col + 17 * col
        dup = side[:at] + bytes([side[at + 1]]) + side[at + 1 :]             # one symbol twice, one missing
        assert Ranges(hs, a, index, dup).run(offset, length) == (CHECKPOINT, b"\xEE" * length, True), col
    dup = side[:other] + bytes([side[other + 1]]) + side[other + 1 :]
    assert Ranges(hs, a, index, dup).run(offset, length) == (DONE, want, True)                  # a checkpoint the range does not use
    assert Ranges(hs, a, index, dup).run(16 * 10, 16 * 100) == (DONE, data[160:1760], True)     # ... and no checkpoint at all: c = 0
    for at in (0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 63):                    # every header field on the device against `ck`
        bad = side[:at] + bytes([side[at] ^ 1]) + side[at + 1 :]
        assert Ranges(hs, a, index, bad, info=info, ck=ck).run(offset, length) == (CHECKPOINT, b"\xEE" * length, True), at
        assert Ranges(hs, a, index, bad, info=info, ck=ck).run(16 * 10, 16) == (CHECKPOINT, b"\xEE" * 16, True), at
    # a permutation, but another one: wrong bytes marked DONE -- the range decode cannot prove content (include/hsrle.h says so)
    swapped = bytearray(side)
    swapped[used], swapped[used + 1] = swapped[used + 1], swapped[used]
    status, got, clean = Ranges(hs, a, index, bytes(swapped)).run(offset, length)
    assert (status, clean) == (DONE, True) and got == G.model_range_decode(a, index, bytes(swapped), offset, length)


def test_index_tampers_inside_the_ranges_stretches(hs, base):
    a, b, data, index, side = base
    offset, length = RANGE
    info = hs.rle8_mmtf128_index_info(index)
    entries = X.unpack_index(index)[3]
    inside = [k for k, e in enumerate(entries) if 128 <= e[1] < 231]
    assert len(inside) >= 2 and entries[inside[0] - 1][1] < 128
    singles = {name: bad for name, bad in X.single_field_tampers(index).items() if any(name.startswith(f"entry{k}_") for k in inside)}
    assert len(singles) == 2 * 8
    for name, bad in singles.items():
        with pytest.raises(X.IndexMismatch):
            G.model_range_decode(a, bad, side, offset, length)
        assert Ranges(hs, a, bad, side, info=info).run(offset, length) == (INDEX, b"\xEE" * length, True), name
    # entries 0 and 1 swapped or doubled: a range whose stretches hold both (rows 64 .. 199; the range above starts behind entry 0 and never reads it)
    structural = X.structural_tampers(a, index)
    offset2, length2 = 16 * 70, 16 * 130
    assert Ranges(hs, a, index, side).run(offset2, length2) == (DONE, data[offset2 : offset2 + length2], True)
    for name in ("swapped", "duplicated_over_neighbour", "duplicated_inserted"):
        with pytest.raises(X.IndexMismatch):
            G.model_range_decode(a, structural[name], side, offset2, length2)
        assert Ranges(hs, a, structural[name], side, info=info).run(offset2, length2) == (INDEX, b"\xEE" * length2, True), name
    assert Ranges(hs, a, X.model_index(b, 64), side, info=info).run(offset, length) == (INDEX, b"\xEE" * length, True)
    for field, value in (("compressedSize", len(a) - 1), ("recordCount", info.recordCount - 1)):         # the index header on the device against `info`
        t = type(info).from_buffer_copy(info)
        setattr(t, field, value)
        ck = hs.rle8_mmtf128_checkpoints_info(side)
        if field == "compressedSize":
            ck.streamSize = value                                            # (the two infos agree: the device has to see it)
        status, got, clean = Ranges(hs, a, index, side, info=t, ck=ck).run(offset, length)
        assert (status, got, clean) == (INDEX, b"\xEE" * length, True), field
    bad = a[:4] + struct.pack("<I", len(a) + 1) + a[8:]                      # the stream header against the arguments
    assert Ranges(hs, bad, index, side).run(offset, length) == (MALFORMED, b"\xEE" * length, True)


def test_an_entry_into_a_body_never_writes_outside(hs, base):
    """e0 has nothing in front of it that vouches for it: pointed into a COPY body it may parse as headers.  Whatever comes of it -- INDEX, or DONE with any
    bytes -- stays inside dOut[0, length)."""
    a, _, data, index, side = base
    info = hs.rle8_mmtf128_index_info(index)
    in_size, stream_size, spacing, entries = X.unpack_index(index)
    for k, (off, row, n, kind) in enumerate(entries):
        if kind != X.COPY:
            continue
        for shift in (1, 2, 3, 5, 17):
            bad = X.pack_index(in_size, stream_size, spacing, entries[:k] + [(off + shift, row, n, kind)] + entries[k + 1 :])
            c = row // 64 * 64
            for offset, length in ((16 * (c + 64) + 3, 16 * 40), (16 * (c + 64), 1), (16 * (c + 70), len(data) - 16 * (c + 70))):
                if offset + length > len(data):
                    continue
                assert G.range_rows(len(data), offset, length, 64)[0] == c + 64
                assert max(j for j, e in enumerate(entries) if e[1] <= c + 64) == k                               # entry k is e0
                status, got, clean = Ranges(hs, a, bad, side, info=info).run(offset, length)
                assert clean and status in (DONE, INDEX), (k, shift, offset)
                if status == INDEX:
                    assert got == b"\xEE" * length, (k, shift, offset)


def test_graph_capture_and_replay(hs, base):
    """One range call captured once, replayed on a second stream, index and checkpoints of the same sizes and counts in the same buffers, the workspace
    refilled with garbage; then the first stream with the second's index (INDEX) and with the second's checkpoints (DONE: other lists, other bytes)."""
    import torch

    a, b, data_a, index_a, side_a = base
    data_b, index_b = T.model_decompress(b), X.model_index(b, 64)
    side_b = model_side(data_b, 64, len(b))
    assert len(a) == len(b) and len(index_a) == len(index_b) and len(side_a) == len(side_b) and data_a != data_b
    offset, length = RANGE
    src, idx, ckp = to_dev(a, 1), to_dev(index_a, 3), to_dev(side_a, 5)
    full, dst = guarded(length, 7)
    info, ck = hs.rle8_mmtf128_index_info(index_a), hs.rle8_mmtf128_checkpoints_info(side_a)
    ws = garbage(hs.rle8_mmtf128_range_workspace_size(length, 64, 64), 9)
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        hs.rle8_mmtf128_decompress_range_dev(src, idx, info, ckp, ck, offset, length, dst, status, ws, stream=side)     # warm-up outside the capture (module load)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        hs.rle8_mmtf128_decompress_range_dev(src, idx, info, ckp, ck, offset, length, dst, status, ws, stream=side)
    put = lambda t, bytes_: t.copy_(torch.from_numpy(np.frombuffer(bytes_, dtype=np.uint8).copy()))
    for stream, index, sidecar, want_status, want in ((b, index_b, side_b, DONE, data_b), (a, index_a, side_a, DONE, data_a), (a, index_b, side_a, INDEX, None),
                                                      (b, index_b, side_b, DONE, data_b)):
        put(src, stream), put(idx, index), put(ckp, sidecar)
        full.fill_(0xEE)
        ws.fill_(0x5A)
        status.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert int(status.item()) == want_status
        assert untouched(full, 7, length)
        got = dst.cpu().numpy().tobytes()
        assert got == (want[offset : offset + length] if want is not None else b"\xEE" * length)


def test_host_calls(hs, base):
    a, b, data, index, side = base
    offset, length = RANGE
    for name, stream, want in [("tamper_base", a, data)] + [(k, *STREAMS[k]) for k in ("no_entry", "long_rle", "under_one_row")]:
        idx = X.model_index(stream, 64)
        rc, built = hs.rle8_mmtf128_checkpoints_build_host(stream + bytes(5), idx, 64)
        assert (rc, built) == (hs.OK, model_side(want, 64, len(stream))), name
        for o, l in ((0, len(want)), (len(want) - 1, 1), (min(16 * 70 + 3, len(want) - 1), min(300, len(want) - min(16 * 70 + 3, len(want) - 1)))):
            assert hs.rle8_mmtf128_decompress_range_host(stream, idx, built, o, l) == (hs.OK, want[o : o + l]), (name, o, l)
    assert hs.rle8_mmtf128_decompress_range_host(a, X.model_index(b, 64), side, offset, length) == (hs.ERR_FORMAT, b"")
    used = 64 + 4096
    assert hs.rle8_mmtf128_decompress_range_host(a, index, side[:used] + bytes([side[used + 1]]) + side[used + 1 :], offset, length) == (hs.ERR_FORMAT, b"")
    assert hs.rle8_mmtf128_checkpoints_build_host(a, X.model_index(b, 64), 64) == (hs.ERR_FORMAT, b"")
    assert hs.rle8_mmtf128_checkpoints_build_host(a, index, 64, cap=len(side) - 1) == (hs.ERR_CAPACITY, b"")
