"""hsrle_compress_mono_dev_enqueue: ONE monolithic reference stream of the 44 codecs whose encoder state at a cut is fixed by the cut (rle8_multi,
rle8_packed_multi; plain / Packed of 2 .. 8 byte symbols; Short with no list or a one-symbol list), encoded without the host in the loop by the
windowed position-parallel encoders in their chunk mode (csrc/hsrle_encodeSpw.hip.h, csrc/hsrle_encode8pw.hip.h).  Bar: the stream equals the
oracle's (= the reference's) byte for byte; its size agrees in its header, the device word and its length; the status says DONE; nothing at or
behind rle_compress_bounds(n) of the output is written; chunks shorter and longer than a 4 KiB window, inputs whose runs end at or near the input's
end, unaligned inputs; a captured HIP graph replayed on new bytes; the synchronous and drop-in paths, which now take the same kernels."""
import random

import numpy as np
import pytest

from hsrle_testlib import CODEC_BY_KEY, SYNTH_RUNS, SYNTH_VIDEO

pytestmark = pytest.mark.gpu

ENQUEUE_KEYS = ["rle8_multi", "rle8_packed_multi", "rle8_multi_short", "rle8_1symlut_short"]
for _W in (16, 24, 32, 48, 64):
    for _v in ("sym", "byte"):
        ENQUEUE_KEYS += [f"rle{_W}_{_v}", f"rle{_W}_{_v}_packed", f"rle{_W}_{_v}_short", f"rle{_W}_1symlut_{_v}_short"]

# one or more of every family and symbol width for the edge cases
EDGE_KEYS = ["rle8_multi_short", "rle8_1symlut_short", "rle16_sym_packed", "rle16_byte", "rle16_sym_short", "rle24_byte_packed", "rle24_1symlut_sym_short",
             "rle32_sym", "rle32_byte_short", "rle32_1symlut_byte_short", "rle48_byte_packed", "rle48_1symlut_byte_short", "rle64_sym_packed", "rle64_byte",
             "rle64_1symlut_sym_short"]
TUNINGS = [0, 64, 100, 1000, None]   # piece sizes G (0: the library's choice; None: 4096 + S -- chunks a little longer than a window)
SLACK = 4096


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    yield hsrle
    hsrle.mono_tuning(0, 0, 0)


@pytest.fixture
def tuned(hs):
    yield hs
    hs.mono_tuning(0, 0, 0)                                                  # (process-global)


def _encode(hs, key, src, fill=0xEE):
    """Enqueue-only encode of the CUDA uint8 tensor src -> (stream bytes, size word, status, slack untouched?)."""
    import torch

    n = src.numel()
    bound = hs.compress_bounds(n)
    dst = torch.full((bound + SLACK,), fill, dtype=torch.uint8, device="cuda")
    ws = hs._scratch(max(hs.mono_compress_workspace_size(key, n), 256), src.device)
    ws.fill_(0xC3)
    status = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    size = torch.full((1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    hs.mono_compress_dev_enqueue(key, src, dst, ws, status, size)
    torch.cuda.synchronize()
    got = int(size.item())
    stream = dst[: max(got, 0)].cpu().numpy().tobytes() if 0 < got <= bound else b""
    untouched = bool((dst[bound:] == fill).all())
    return stream, got, int(status.item()), untouched


def _check(hs, oracle, key, data, src, what, want=None):
    if want is None:
        want = oracle.compress(CODEC_BY_KEY[key], bytes(data))
    stream, size, status, untouched = _encode(hs, key, src)
    assert status == hs.MONO_DONE, f"{key} {what}: status {status}"
    assert size == len(want), f"{key} {what}: size word {size}, oracle {len(want)}"
    assert int.from_bytes(stream[4:8], "little") == len(want), f"{key} {what}: header size"
    assert stream == want, f"{key} {what}: stream differs from the oracle's"
    assert untouched, f"{key} {what}: bytes at or behind rle_compress_bounds(n) written"


@pytest.mark.parametrize("key", ENQUEUE_KEYS)
@pytest.mark.parametrize("kind", [SYNTH_RUNS, SYNTH_VIDEO])
def test_every_accepted_codec(hs, oracle, key, kind):
    import torch

    codec = CODEC_BY_KEY[key]
    data = oracle.synth(kind, codec.S, 41, (5 << 20) + 1237 + 2 * codec.S)
    _check(hs, oracle, key, data.tobytes(), torch.from_numpy(data).cuda(), f"synth {kind}")


def _runs(rng, n, S, sym_pool):
    """Literal stretches and runs of a few S-byte symbols, run lengths around the store thresholds, some not a multiple of S."""
    out = bytearray()
    while len(out) < n:
        out += bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 2, 5, 17, 40])))
        s = rng.choice(sym_pool)
        out += s * rng.choice([1, 2, 3, 5, 8, 12, 13, 20, 40, 300]) + s[: rng.randrange(S)]
    return bytearray(out[:n])


def _edge_inputs(S, n, seed):
    rng = random.Random(seed)
    pool = [bytes(rng.randrange(256) for _ in range(S)) for _ in range(3)]
    cases = [("random", bytearray(rng.randrange(256) for _ in range(n))), ("zeros", bytearray(n)), ("runs", _runs(rng, n, S, pool))]
    # a run that ends exactly at the input's end, and 1 .. S - 1 bytes in front of it
    for t in range(S):
        d = _runs(rng, n, S, pool)
        sym = pool[0]
        L = min(n - t, S * ((3 * S + 20) // S))                          # (whole symbols: the run ends where its last period does)
        if L > 0:
            d[n - t - L : n - t] = (sym * (L // S + 1))[:L]
        for i in range(max(n - t, 0), n):
            d[i] = (sym[0] + 1 + i) & 0xFF
        cases.append((f"run ends {t} before the end", d))
    if n > 4096:
        d = _runs(rng, n, S, pool)
        for edge in range(4096, n, 4096):
            a, b = edge - rng.randrange(1, 60), min(n, edge + rng.randrange(0, 60))
            d[a:b] = (pool[1] * ((b - a) // S + 1))[: b - a]
        cases.append(("runs across 4 KiB edges", d))
    return cases


@pytest.mark.parametrize("key", EDGE_KEYS)
def test_chunk_and_window_edges(tuned, oracle, key):
    import torch

    hs = tuned
    S = CODEC_BY_KEY[key].S
    sizes = sorted({n for n in (1, S - 1, S, S + 10, S + 11, 4095, 4096, 4097, 4096 + S - 1, 8192 + S - 1, 12 * 1024 + 5, 65535) if n >= 1})
    cases = [(n, what, bytes(data), oracle.compress(CODEC_BY_KEY[key], bytes(data))) for n in sizes for what, data in _edge_inputs(S, n, 1000 * n + S)]
    k = 0
    for G in TUNINGS:
        hs.mono_tuning(0, 4096 + S if G is None else G, 0)
        for n, what, data, want in cases:
            off = 1 + k % 7                                                  # src at byte offsets 1 .. 7
            k += 1
            buf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
            buf[off : off + n] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            _check(hs, oracle, key, data, buf[off : off + n], f"n={n} {what} G={G} offset {off}", want)


@pytest.mark.parametrize("key", ENQUEUE_KEYS)
def test_run_to_the_end_across_a_window_edge(tuned, oracle, key):
    """The input ends 1 .. S - 1 bytes into a 4 KiB window with a run that reaches its last byte: the run's match stretch ends in the window in front,
    and the last window's terminator must still say that the stream ended on a run (the reference's fuzzer shape: [r][s][r][s][r][s x L])."""
    import torch

    hs = tuned
    S = CODEC_BY_KEY[key].S
    rng = random.Random(S)
    for G in (0, 64, 1000):
        hs.mono_tuning(0, G, 0)
        for n in sorted({4096 * k + r for k in (1, 2, 3) for r in range(0, S + 1)}):
            for sym in (bytes([rng.randrange(256)]) * S, bytes(rng.randrange(256) for _ in range(S))):
                head = bytes([rng.randrange(256), sym[0], rng.randrange(256), sym[0], rng.randrange(256)])
                data = head + (sym * (n // S + 1))[: n - len(head)]
                _check(hs, oracle, key, data, torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(), f"n={n} G={G}")
                tail = (n - len(head)) % S                                   # (and a run that ends exactly on a whole symbol at the input's end)
                if tail:
                    data = head + bytes(tail) + (sym * (n // S + 1))[: n - len(head) - tail]
                    _check(hs, oracle, key, data, torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(), f"n={n} G={G} whole symbols")


@pytest.mark.parametrize("key", ["rle32_byte_packed", "rle64_sym", "rle16_1symlut_byte_short"])
def test_graph_capture_and_replay(hs, oracle, key):
    """Captured once on a side stream, replayed on new input bytes with garbage in dst and the workspace: every replay is the oracle's stream."""
    import torch

    codec = CODEC_BY_KEY[key]
    n = (6 << 20) + 29
    inputs = [oracle.synth(SYNTH_RUNS, codec.S, 51, n), oracle.synth(SYNTH_VIDEO, codec.S, 52, n), oracle.synth(SYNTH_RUNS, codec.S, 53, n)]
    src = torch.from_numpy(inputs[0]).cuda()
    dst = torch.empty(hs.compress_bounds(n) + 64, dtype=torch.uint8, device="cuda")
    ws = torch.empty(hs.mono_compress_workspace_size(key, n), dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hs.mono_compress_dev_enqueue(key, src, dst, ws, status, size)     # warm-up outside the capture (module load)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        hs.mono_compress_dev_enqueue(key, src, dst, ws, status, size)
    for data in (inputs[1], inputs[2], inputs[0]):
        src.copy_(torch.from_numpy(data))
        dst.fill_(0xEE)
        ws.fill_(0xC3)
        size.zero_()
        status.fill_(77)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = oracle.compress(codec, data.tobytes())
        assert int(status.item()) == hs.MONO_DONE
        assert int(size.item()) == len(want)
        assert dst[: len(want)].cpu().numpy().tobytes() == want


@pytest.mark.parametrize("key", ["rle16_sym", "rle24_byte_packed", "rle32_sym_packed", "rle48_byte", "rle64_byte_packed", "rle16_1symlut_sym_short",
                                 "rle32_byte_short", "rle64_1symlut_byte_short", "rle8_multi_short", "rle8_1symlut_short"])
def test_synchronous_and_dropin_paths(tuned, oracle, key):
    """hsrle_compress_mono_dev and the drop-in rle*_compress take the windowed chunk mode too: the oracle's stream under small pieces."""
    import torch

    hs = tuned
    codec = CODEC_BY_KEY[key]
    rng = random.Random(7)
    pool = [bytes(rng.randrange(256) for _ in range(codec.S)) for _ in range(4)]
    cases = [bytes(_runs(rng, n, codec.S, pool)) for n in (3000, 40000, 150001)] + [oracle.synth(SYNTH_VIDEO, codec.S, 3, 300007).tobytes()]
    for G in (64, 100, 1000, 0):
        hs.mono_tuning(0, G, 0)
        for d in cases:
            want = oracle.compress(codec, d)
            size, stream = hs.call_dropin(codec.cname, d, hs.compress_bounds(len(d)))
            assert size == len(want) and stream == want, f"{key} drop-in len {len(d)} G={G}"
            got = hs.mono_compress_dev(key, torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda())
            assert got.cpu().numpy().tobytes() == want, f"{key} hsrle_compress_mono_dev len {len(d)} G={G}"


def test_one_symbol_list_encode_needs_no_rounds(hs, oracle):
    """The list in front of a chunk of a one-symbol-list Short codec is the cut's symbol: no guesses, no rounds -- the stats read zero."""
    import torch

    src = hs.synth(SYNTH_RUNS, 4, 8, 8 << 20, device="cuda")
    hs.mono_compress_dev("rle32_3symlut_sym", src)                        # (a list codec first: its stats may be anything)
    got = hs.mono_compress_dev("rle32_1symlut_sym_short", src)
    assert got.cpu().numpy().tobytes() == oracle.compress(CODEC_BY_KEY["rle32_1symlut_sym_short"], src.cpu().numpy().tobytes())
    assert hs.mono_encode_stats() == (0, 0, 0, 0)


def test_bad_tensors_are_refused_before_the_call(hs):
    import torch

    n = 1 << 16
    src = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dst = torch.empty(hs.compress_bounds(n) + 64, dtype=torch.uint8, device="cuda")
    ws = torch.empty(hs.mono_compress_workspace_size("rle32_sym", n), dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    bad = [(src.cpu(), dst, ws, status), (src, dst.to(torch.int16), ws, status), (src, dst, ws[::2], status), (src, dst, ws, torch.zeros(2, dtype=torch.uint8, device="cuda")),
           (src, dst, ws, status.cpu())]
    for a in bad:
        with pytest.raises(hs.HsrleError):
            hs.mono_compress_dev_enqueue("rle32_sym", *a)
    with pytest.raises(hs.HsrleError):
        hs.mono_compress_dev_async("rle8_multi", src, dst, ws, torch.zeros(1, dtype=torch.uint8, device="cuda"))
    with pytest.raises(hs.HsrleError) as e:
        hs.mono_compress_dev_enqueue("rle32_3symlut_sym", src, dst, ws, status)
    assert e.value.status == hs.ERR_UNSUPPORTED
