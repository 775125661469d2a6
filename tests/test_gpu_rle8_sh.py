"""rle8_sh on the GPU (csrc/hsrle_rle8sh.hip.h) against the sequential models (tests/rle8_sh_testlib.py, themselves held against the compiled
reference by test_rle8_sh_model.py).  Encode: the stream equals the model's -- the reference's -- byte for byte.  Decode: the reference's stored
streams, the model's streams and streams written from the grammar, with what no encoder writes: literals that promote behind S / T, FILL large
counts through the 32-bit wrap, a gap between body and bits.  Every tuning value gives the same bytes.  Malformed streams are refused by the
walk's bounds checks before anything is written."""
import json

import numpy as np
import pytest

import rle8_sh_testlib as T
from mmtf_testlib import video_shaped

pytestmark = pytest.mark.gpu

GUARD = 4096
DONE, MALFORMED, CAPACITY = 0, 1, 2
INPUTS = T.input_set()
_STREAM = {}
LAST_WORDS = [None, None]          # (fallback ran, failed proofs) of the last decompress_dev


def model_stream(name, data):
    if name not in _STREAM:
        _STREAM[name] = T.model_compress(data)[0]
    return _STREAM[name]


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    hsrle.rle8_sh_tuning(0, 0, 0)
    yield hsrle
    hsrle.rle8_sh_tuning(0, 0, 0)


@pytest.fixture
def tuned(hs):
    yield hs
    hs.rle8_sh_tuning(0, 0, 0)                                                  # (process-global)


def to_dev(data, offset=0):
    import torch

    t = torch.zeros(len(data) + offset + 64, dtype=torch.uint8, device="cuda")[offset : offset + len(data)]
    t.copy_(torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()))
    return t


def compress_dev(hs, data, offsets=(0, 0, 0), cap=None):
    """(size word, status word, the out buffer's bytes, nothing written outside [0, size)?).  Out buffer: 0xEE, workspace: 0xC3 garbage."""
    import torch

    n = len(data)
    cap = hs.rle8_sh_capacity(n) if cap is None else cap
    src = to_dev(data, offsets[0])
    lead = GUARD + offsets[1]
    full = torch.full((lead + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dst = full[lead : lead + cap]
    ws = torch.full((hs.rle8_sh_workspace_size(0, n) + offsets[2],), 0xC3, dtype=torch.uint8, device="cuda")[offsets[2] :]
    words = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    hs.rle8_sh_compress_dev(src, dst, words[0:1], words[1:2], ws)
    torch.cuda.synchronize()
    size, status = (int(x) for x in words.cpu().numpy())
    host = full.cpu().numpy()
    clean = bool((host[:lead] == 0xEE).all() and (host[lead + size :] == 0xEE).all())
    return size, status, host[lead : lead + cap].tobytes(), clean


def check_encode(hs, name, data, want, offsets=(0, 0, 0)):
    size, status, out, clean = compress_dev(hs, data, offsets)
    assert (status, size) == (DONE, len(want)), name
    assert out[:size] == want, f"{name}: the stream differs from the model's"
    assert clean, f"{name}: compress wrote outside [0, size)"


def decompress_dev(hs, stream, n, offsets=(0, 0, 0)):
    """(status word, output bytes, canary on both sides of the output intact?).  Output buffer: 0xEE, workspace: 0xC3 garbage."""
    import torch

    src = to_dev(stream, offsets[0])
    lead = GUARD + offsets[1]
    full = torch.full((lead + n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dst = full[lead : lead + n]
    ws = torch.full((hs.rle8_sh_workspace_size(1, n) + offsets[2],), 0xC3, dtype=torch.uint8, device="cuda")[offsets[2] :]
    status = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    hs.rle8_sh_decompress_dev(src, dst, status, ws)
    torch.cuda.synchronize()
    LAST_WORDS[:] = hs.rle8_sh_decode_words(ws) if int(status.item()) == DONE else (None, None)
    host = full.cpu().numpy()
    clean = bool((host[:lead] == 0xEE).all() and (host[lead + n :] == 0xEE).all())
    return int(status.item()), host[lead : lead + n].tobytes(), clean


def check_decode(hs, name, stream, want, offsets=(0, 0, 0)):
    status, back, clean = decompress_dev(hs, stream, len(want), offsets)
    assert status == DONE, name
    assert back == want, f"{name}: decode differs"
    assert clean, f"{name}: wrote outside the output"


@pytest.mark.parametrize("name", list(INPUTS))
def test_compress_gives_the_models_bytes(hs, name):
    data, want = INPUTS[name], model_stream(name, INPUTS[name])
    check_encode(hs, name, data, want)
    assert hs.rle8_sh_compress(data) == (len(want), want), name


def test_compress_gives_the_references_stored_bytes(hs):
    for v in golden():
        check_encode(hs, v["name"], bytes.fromhex(v["input"]), bytes.fromhex(v["stream"]))


@pytest.mark.parametrize("name", list(INPUTS))
def test_decode_of_the_encoder_models_streams(hs, name):
    check_decode(hs, name, model_stream(name, INPUTS[name]), INPUTS[name])


def golden():
    with open(T.GOLDEN) as f:
        return json.load(f)["vectors"]


def test_decode_of_the_references_stored_streams(hs):
    for v in golden():
        data, stream = bytes.fromhex(v["input"]), bytes.fromhex(v["stream"])
        check_decode(hs, v["name"], stream, data)
        assert hs.rle8_sh_decompress(stream, len(data)) == (len(data), data), v["name"]


GRAMMAR = T.grammar_streams()


@pytest.mark.parametrize("name", list(GRAMMAR))
def test_decode_of_grammar_written_streams(hs, name):
    stream = GRAMMAR[name]
    want = T.model_decompress(stream)
    assert want is not None
    check_decode(hs, name, stream, want)
    assert hs.rle8_sh_decompress(stream, len(want) + 5) == (len(want), want)


@pytest.mark.parametrize("stretch,window,serial", ((1, 0, 0), (0, 64, 0), (1, 64, 1), (7, 80, 0), (4096, 1008, 0), (0, 0, 1), (0, 0, 0)))
def test_both_decode_paths_and_every_tuning_value_give_the_same_bytes(tuned, stretch, window, serial):
    """stretch 1: every word of the bit stream is a record of its own; window 64: the smallest walk window, an edge every 48 bytes of bits;
    serial 1: the serial symbol pass forced.  Without it an encoder-made stream never takes the fallback: its guess holds."""
    tuned.rle8_sh_tuning(stretch, window, serial)
    for name, data in INPUTS.items():
        check_decode(tuned, f"{name} stretch {stretch} window {window} serial {serial}", model_stream(name, data), data)
        assert LAST_WORDS == [serial, 0], name
    for name, stream in GRAMMAR.items():
        check_decode(tuned, f"{name} stretch {stretch} window {window} serial {serial}", stream, T.model_decompress(stream))
        assert LAST_WORDS[0] == (1 if serial or name in PROMOTES_BEHIND_S_T else 0), name


PROMOTES_BEHIND_S_T = ("literal_behind_S_promotes", "literal_behind_T_promotes")


def test_a_literal_that_promotes_behind_s_or_t_takes_the_fallback(hs):
    """No encoder writes these: the guess fails, a proof says so, the serial pass and a second expansion give the reference's bytes."""
    for name in PROMOTES_BEHIND_S_T:
        check_decode(hs, name, GRAMMAR[name], T.model_decompress(GRAMMAR[name]))
        assert LAST_WORDS[0] == 1 and LAST_WORDS[1] >= 1, name
    check_decode(hs, "three_equal_literals", GRAMMAR["three_equal_literals"], T.model_decompress(GRAMMAR["three_equal_literals"]))
    assert LAST_WORDS == [0, 0]                                               # (literals behind literals promote for sure: no guess in that)
    # the same literal far into a long stream, behind many stretch records, with stretches after it that depend on the promotion
    Z, S, Tk = ("Z",), ("S",), ("T",)
    # (second = 0x32 and third = 0x31 behind the head; S gives 0x32, the literal 0x32 behind it promotes: third becomes 0x32, and every T shows it)
    head = ([Z] * 5 + [("L", 0x31), ("L", 0x31), S, Tk, ("L", 0x32), ("L", 0x32)]) * 200
    tokens = head + [("L", 0x40), S, ("L", 0x32)] + ([Z] * 7 + [S, Tk, ("L", 0x33), Tk, S]) * 200 + [("END",)]
    stream = T.write_stream(sum(1 for _ in tokens) - 1, tokens)
    check_decode(hs, "late_promotion_behind_S", stream, T.model_decompress(stream))
    assert LAST_WORDS[0] == 1 and LAST_WORDS[1] >= 1


@pytest.mark.parametrize("offsets", ((1, 3, 5), (3, 17, 1), (17, 1, 3)))
def test_odd_addresses(hs, offsets):
    for name in ("raw_263", "r_rich_900_encoded", "alphabet4_3000", "random_3000", "r_run_of_270", "random_1"):
        check_encode(hs, name, INPUTS[name], model_stream(name, INPUTS[name]), offsets)
        check_decode(hs, name, model_stream(name, INPUTS[name]), INPUTS[name], offsets)
    check_decode(hs, "raw_copies_cross_chunks", GRAMMAR["raw_copies_cross_chunks"], T.model_decompress(GRAMMAR["raw_copies_cross_chunks"]), offsets)


def test_malformed_streams_are_refused_before_any_write(hs):
    good, bad = T.malformed_streams()
    assert decompress_dev(hs, good, 30)[0] == DONE
    for name, (n, stream) in bad.items():
        if name != "header_size_is_not_the_output_size":
            assert T.model_decompress(stream) is None, name
        status, out, clean = decompress_dev(hs, stream, n)
        assert status == MALFORMED, name
        assert clean and out == b"\xEE" * n, f"{name}: the output or the canary around it was touched"
        if name != "header_size_is_not_the_output_size":
            assert hs.rle8_sh_decompress(stream, n + 64) == (0, b""), name


def test_capacity_one_byte_short(hs):
    """outCapacity one byte under the stream: CAPACITY, size word 0, nothing written.  (Random bytes: the stream is n + 18, above the least
    capacity the call accepts, n + 8.)"""
    import random

    data = random.Random(8).randbytes(2000)
    want = T.model_compress(data)[0]
    assert len(want) == len(data) + 18
    size, status, out, clean = compress_dev(hs, data, cap=len(want) - 1)
    assert (size, status) == (0, CAPACITY)
    assert clean and out == b"\xEE" * len(out)
    size, status, out, clean = compress_dev(hs, data, cap=len(want))
    assert (size, status, out, clean) == (len(want), DONE, want, True)
    assert hs.rle8_sh_compress(data, out_cap=len(want) - 1) == (0, b"")
    assert hs.rle8_sh_compress(data, out_cap=len(want)) == (len(want), want)


def test_the_derived_capacity_suffices(hs):
    """hsrle_rle8_sh_capacity (include/hsrle.h has the derivation) on random bytes, on short coded stretches between FILLs and on the input built to
    grow: raw blocks of 263 bytes between runs of 10."""
    import random

    rng = random.Random(4)
    inputs = {f"random_{n}": rng.randbytes(n) for n in (1, 7, 8, 263, 270, 40000)}
    inputs["short_coded_stretches"] = T.short_coded_stretches(30000)
    inputs["raw_blocks_between_changes"] = T.raw_blocks_between_changes(273 * 150)
    inputs["marginal_encoded_spans"] = T.marginal_encoded_spans(5000)        # 1.875 bytes per block of 416: the worst case per byte
    for name, data in inputs.items():
        want = T.model_compress(data)[0]
        assert len(want) <= hs.rle8_sh_capacity(len(data)), name
        check_encode(hs, name, data, want)
    worst = inputs["marginal_encoded_spans"]
    assert len(T.model_compress(worst)[0]) - len(worst) > 150 > 21            # (far past the constant slack)
    assert hs.rle8_sh_compress(worst) == (len(T.model_compress(worst)[0]), T.model_compress(worst)[0])
    grown = inputs["raw_blocks_between_changes"]
    assert len(T.model_compress(grown)[0]) > hs.rle8_sh_bounds(len(grown)) + 100          # (the reference's bound is far from one)


def test_drop_in_function(hs):
    assert hs.rle8_sh_bounds(1000) == 1013 and hs.rle8_sh_bounds((1 << 30) + 1) == 0
    assert hs.rle8_sh_compress(b"")[0] == 0
    assert hs.rle8_sh_compress(bytes(32), out_cap=39)[0] == 0
    for name in ("random_1", "random_16", "alphabet3_1000", "r_rich_417_encoded", "raw_262", "random_3000"):
        data, stream = INPUTS[name], model_stream(name, INPUTS[name])
        assert hs.rle8_sh_decompress(stream, len(data)) == (len(data), data), name
        assert hs.rle8_sh_decompress(stream + bytes(7), len(data) + 9) == (len(data), data), name
        assert hs.rle8_sh_decompress(stream, len(data) - 1)[0] == 0, name                   # header inSize > outSize
        assert hs.rle8_sh_decompress(stream[:-1], len(data))[0] == 0, name                  # header streamSize > inSize


def big_inputs():
    n = 3 << 20
    return {"runs_3MiB": T.geometric_runs(n, 8, 11, mean=40), "video_3MiB": video_shaped(n)}


@pytest.mark.parametrize("name", ("runs_3MiB", "video_3MiB"))
def test_three_mebibytes(hs, name):
    """Crosses the walk's windows many times; the expansion runs over thousands of workgroups."""
    data = big_inputs()[name]
    want = T.model_compress(data)[0]
    check_encode(hs, name, data, want)
    check_decode(hs, name, want, data)


def test_stream_of_tiny_items(hs):
    """2^17 records and more: one Z and a FILL large of ONE byte (through the wrap) that changes R, again and again."""
    pairs = (1 << 16) + 5
    stream = T.tiny_items(pairs)
    want = bytearray()
    r = 0x7F
    for i in range(pairs):
        want.append(r)
        r = i % 251
        want.append(r)
    check_decode(hs, "tiny_items", stream, bytes(want))


def test_graph_capture_and_replay(hs):
    """Compress and decompress captured once on a side stream and replayed on new bytes, the workspaces refilled with garbage before each replay.
    (The decode's stream length is part of the captured call: the replays' inputs are chosen to give streams of the same size.)"""
    import torch

    n = 700
    inputs = [bytes([a]) * 20 + T.noise(300, a, avoid=(0x7F,)) + b"\x7F" * 80 + T.noise(300, a + 9, avoid=(0x7F,)) for a in (1, 2, 3)]
    streams = [T.model_compress(d)[0] for d in inputs]
    assert len({len(s) for s in streams}) == 1
    size, cap = len(streams[0]), hs.rle8_sh_capacity(n)
    src = to_dev(inputs[0])
    enc = torch.full((cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dec = torch.full((n + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    ws1 = torch.full((hs.rle8_sh_workspace_size(0, n),), 0xC3, dtype=torch.uint8, device="cuda")
    ws2 = torch.full((hs.rle8_sh_workspace_size(1, n),), 0xC3, dtype=torch.uint8, device="cuda")
    words = torch.full((3,), -1, dtype=torch.int32, device="cuda")

    def both(stream):
        hs.rle8_sh_compress_dev(src, enc[:cap], words[0:1], words[1:2], ws1, stream=stream)
        hs.rle8_sh_decompress_dev(enc[:size], dec[:n], words[2:3], ws2, stream=stream)

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        both(side)                                                           # warm-up outside the capture (module load)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        both(side)
    for data, want in zip(inputs[1:], streams[1:]):
        src.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
        enc.fill_(0xEE)
        dec.fill_(0xEE)
        ws1.fill_(0x5A)
        ws2.fill_(0xA5)
        words.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        e, d = enc.cpu().numpy(), dec.cpu().numpy()
        assert [int(x) for x in words.cpu().numpy()] == [size, DONE, DONE]
        assert e[:size].tobytes() == want
        assert d[:n].tobytes() == data
        assert (e[size:] == 0xEE).all() and (d[n:] == 0xEE).all()
