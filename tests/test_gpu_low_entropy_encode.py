"""The ENCODERS of the low-entropy codec and of rle8m (csrc/hsrle_rle8m.hip.h, csrc/hsrle_capi_low_entropy.h) on inputs built around the places where they
decide (tests/low_entropy_stats.py): run statistics word for word against the model, streams byte for byte against the oracle, the device entry
hsrle_low_entropy_compress_dev_async with a garbage workspace, at odd addresses, between guards, under graph capture and at its capacity rule, and the
lane-per-section rle8m encoder (131 072 sections and more)."""
import ctypes

import numpy as np
import pytest

import low_entropy_stats as S

pytestmark = pytest.mark.gpu

GUARD = 4096
LE_NAMES = ("rle8_low_entropy_compress", "rle8_low_entropy_short_compress", "rle8_low_entropy_compress_only_max_frequency", "rle8_low_entropy_short_compress_only_max_frequency")
WORD = 0x5A5A5A5A     # what the words next to the status word hold


class CompressInfo(ctypes.Structure):
    _fields_ = [("rle", ctypes.c_uint8 * 256), ("symbolsByProb", ctypes.c_uint8 * 256), ("symbolCount", ctypes.c_uint8)]


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    return hsrle


def max_len_of(variant):
    return 32 if variant & 1 else 255


def to_dev(data, offset=0):
    import torch

    t = torch.zeros(data.size + offset + 64, dtype=torch.uint8, device="cuda")[offset : offset + data.size]
    t.copy_(torch.from_numpy(data if data.flags.writeable else data.copy()))
    return t


class Call:
    """One hsrle_low_entropy_compress_dev_async: input, output and workspace start `offsets` bytes (the workspace: 16 bytes each) off their allocations, the
    output between two guards of 0xEE, the workspace 0xC3 garbage, the status word between two other words."""

    def __init__(self, hs, data, offsets=(0, 0, 0), cap=None, ws_short=0):
        import torch

        self.hs, self.n = hs, data.size
        self.cap = hs.low_entropy_bounds(self.n) if cap is None else cap
        self.src = to_dev(data, offsets[0])
        self.lead = GUARD + offsets[1]
        self.buf = torch.full((self.lead + self.cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
        self.dst = self.buf[self.lead : self.lead + self.cap]
        wo = 16 * offsets[2]
        self.ws = torch.full((hs.low_entropy_workspace_size(self.n) + wo - ws_short,), 0xC3, dtype=torch.uint8, device="cuda")[wo:]
        self.words = torch.full((3,), WORD, dtype=torch.int32, device="cuda")

    def run(self, variant, stream=None):
        return self.hs.low_entropy_compress_dev(self.src, variant, self.dst, self.ws, self.words[1:2], stream=stream)

    def refill(self, ws_byte):
        self.buf.fill_(0xEE)
        self.ws.fill_(ws_byte)
        self.words.fill_(WORD)

    def verdict(self, want, check_decode=True):
        """None, or what is wrong with the finished call: status word 0, its neighbours and the guards untouched, the first u32 the size, the stream the
        oracle's, and the stream decodes to the input."""
        import torch

        words = [int(x) for x in self.words.cpu().numpy()]
        out = self.buf.cpu().numpy()
        if not ((out[: self.lead] == 0xEE).all() and (out[self.lead + self.cap :] == 0xEE).all()):
            return "a guard was written"
        if want is None:                                                   # the oracle's stream outgrows the bound: the status word says so
            return None if words[0] == words[2] == WORD and words[1] != 0 else f"the oracle's stream outgrows the bound, status words {words}"
        if words != [WORD, 0, WORD]:
            return f"status words {words}"
        size = int(out[self.lead : self.lead + 4].view("<u4")[0])
        if size != len(want):
            return f"size {size}, the oracle's {len(want)}"
        if out[self.lead : self.lead + size].tobytes() != want:
            return "stream differs from the oracle's"
        if check_decode:
            stream = self.dst[:size].clone()
            back = torch.full((self.n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            dws = torch.full((self.hs.low_entropy_decompress_workspace_size(size),), 0xC3, dtype=torch.uint8, device="cuda")
            rc, got = self.hs.low_entropy_decompress_dev(stream, back[: self.n], dws)
            if (rc, got) != (self.hs.OK, self.n) or not torch.equal(back[: self.n], self.src) or not bool((back[self.n :] == 0xA5).all()):
                return f"decode: code {rc}, {got} bytes"
        return None


def stats_verdict(hs, ws, data, max_len):
    prob, pcount = hs.encode_stats_words(ws)
    want_prob, want_pcount = S.stats(data, max_len)
    bad = [f"prob[{s}] {prob[s]} for {want_prob[s]}" for s in np.flatnonzero(prob != want_prob)] + [f"pcount[{s}] {pcount[s]} for {want_pcount[s]}" for s in np.flatnonzero(pcount != want_pcount)]
    return ", ".join(bad[:6]) if bad else None


def check_unsectioned(hs, oracle, fixtures, variants=range(4), offsets=(0, 0, 0)):
    """D1 + D2 for hsrle_low_entropy_compress_dev_async: every one of the 512 statistics words, and the stream."""
    import torch

    bad = []
    for k, f in enumerate(fixtures):
        call = Call(hs, f.data, (((offsets[0] + 2 * k) % 32) | 1, ((offsets[1] + 6 * k) % 32) | 1, (offsets[2] + k) % 8) if any(offsets) else offsets)   # odd, and not the same for every input
        for variant in variants:
            call.refill(0xC3)
            rc = call.run(variant)
            torch.cuda.synchronize()
            if rc != hs.OK:
                bad.append(f"{f.name} variant {variant}: code {rc}")
                continue
            for what in (stats_verdict(hs, call.ws, f.data, max_len_of(variant)), call.verdict(oracle.low_entropy_compress(variant, f.bytes))):
                if what:
                    bad.append(f"{f.name} variant {variant}: {what}")
    assert not bad, f"{len(bad)} findings, the first: {bad[:8]}"


def check_rle8m_counts(hs, fixtures, section_counts=(1, 7, 64)):
    """D1 for hsrle_rle8m_compress_dev_async: the statistics are over the whole input whatever the section count."""
    import torch

    bad = []
    for f in fixtures:
        src = to_dev(f.data, 1)
        want = [a.copy() for a in S.stats(f.data, 255)]
        for sections in section_counts:
            if f.data.size < sections:
                continue
            dst = torch.empty(hs.rle8m_bounds(sections, f.data.size), dtype=torch.uint8, device="cuda")
            ws = torch.full((hs.rle8m_workspace_size(f.data.size, sections),), 0xC3, dtype=torch.uint8, device="cuda")
            status = torch.ones(1, dtype=torch.int32, device="cuda")
            hs.rle8m_compress_async(src, sections, dst, ws, status)
            torch.cuda.synchronize()
            prob, pcount = hs.encode_stats_words(ws)
            if not (np.array_equal(prob, want[0]) and np.array_equal(pcount, want[1])):
                bad.append(f"{f.name} x{sections}: {stats_verdict(hs, ws, f.data, 255)}")
    assert not bad, f"{len(bad)} findings, the first: {bad[:8]}"


def check_host_names(hs, oracle, fixtures):
    """The same inputs behind the reference's names (host pointers): the four encoders write the oracle's stream -- the model's header in it -- and
    rle8_low_entropy_get_compress_info[_only_max_frequency] return the model's tables."""
    lib = hs.lib()
    getters = []
    for name in ("rle8_low_entropy_get_compress_info", "rle8_low_entropy_get_compress_info_only_max_frequency"):
        getters.append(getattr(lib, name))
    bad = []
    for f in fixtures:
        n = f.data.size
        for variant in range(4):
            head = S.model_header(f.data, max_len_of(variant), variant >> 1)
            size, got = hs.call_dropin(LE_NAMES[variant], f.bytes, hs.low_entropy_bounds(n))
            want = oracle.low_entropy_compress(variant, f.bytes)       # (None: the stream outgrows the bound, and the call returns 0)
            if (size != 0) if want is None else (got != want or got[8 : 8 + len(head)] != head):
                bad.append(f"{f.name}: {LE_NAMES[variant]}")
        prob, pcount = S.stats(f.data, 255)
        for only_max, getter in enumerate(getters):
            info = CompressInfo()
            flags, order, count = S.tables(prob, pcount, only_max)
            if not getter(f.data.ctypes.data, n, ctypes.byref(info)) or bytes(info) != flags.tobytes() + order.tobytes() + bytes([count]):
                bad.append(f"{f.name}: get_compress_info, only_max {only_max}")
    assert not bad, f"{len(bad)} findings, the first: {bad[:8]}"


# ---- the small fixtures (A1, A2, A4), a family per case ----

FAMILIES = ("a1.m255", "a1.m32", "a1.final", "a1.first", "a2.m255", "a2.m32", "a2.saved.m255", "a2.saved.m32", "a2.final", "a4")


def family(name):
    pool = S.fixtures_a1() if name.startswith("a1") else S.fixtures_a2() if name.startswith("a2") else S.fixtures_a4()
    mine = [f for f in pool if f.name.startswith(name)]
    assert mine
    return mine


def test_the_families_are_all_small_fixtures():
    names = [f.name for f in S.fixtures_small()]
    assert sorted(names) == sorted({f.name for fam in FAMILIES for f in family(fam)})


@pytest.mark.parametrize("name", FAMILIES)
def test_counts_and_streams_of_the_threshold_inputs(hs, oracle, name):
    check_unsectioned(hs, oracle, family(name), offsets=(1, 3, 1))


@pytest.mark.parametrize("name", FAMILIES)
def test_rle8m_counts_of_the_threshold_inputs(hs, name):
    check_rle8m_counts(hs, family(name))


@pytest.mark.parametrize("name", FAMILIES + ("a5",))
def test_host_names_on_the_threshold_inputs(hs, oracle, name):
    check_host_names(hs, oracle, S.fixtures_a5() if name == "a5" else family(name))


@pytest.mark.parametrize("offsets", ((0, 0, 0), (1, 3, 1), (3, 17, 5), (17, 1, 3)))
def test_streams_at_the_cut_edges(hs, oracle, offsets):
    check_unsectioned(hs, oracle, S.fixtures_a5(), offsets=offsets)


# ---- scan and grid edges (A3) ----


@pytest.mark.parametrize("k", range(5))
def test_counts_and_streams_at_the_scan_edges(hs, oracle, k):
    f = S.fixtures_a3_mid()[k]
    check_unsectioned(hs, oracle, [f], offsets=(1, 3, 1))
    check_rle8m_counts(hs, [f], (7,))


@pytest.mark.parametrize("k", range(2))
def test_counts_and_streams_across_the_scan_carry(hs, oracle, k):
    f = S.fixtures_a3_carry()[k]
    check_unsectioned(hs, oracle, [f], offsets=(3, 1, 3))
    check_rle8m_counts(hs, [f], (7,))


@pytest.fixture(scope="module")
def big():
    return S.fixture_a3_big()


@pytest.mark.parametrize("variant", range(4))
def test_counts_and_stream_where_a_wave_takes_a_second_piece(hs, oracle, big, variant):
    """(129 << 20) + 4099 bytes: 33 026 pieces on 32 768 waves."""
    import torch

    call = Call(hs, big.data, (1, 3, 1))
    assert call.run(variant) == hs.OK
    torch.cuda.synchronize()
    assert stats_verdict(hs, call.ws, big.data, max_len_of(variant)) is None
    assert call.verdict(oracle.low_entropy_compress(variant, big.bytes)) is None


# ---- the entry point itself ----


def test_capacity_and_argument_rule(hs):
    """Refused on the host, and then nothing is launched: output, guards, workspace and status stay as they were."""
    import torch

    data = S.fixtures_a5()[0].data
    n, bound = data.size, hs.low_entropy_bounds(data.size)
    assert bound == n + 32 + 1 + 256 + 8

    def untouched(call):
        torch.cuda.synchronize()
        return bool((call.buf == 0xEE).all()) and bool((call.ws == 0xC3).all()) and [int(x) for x in call.words.cpu().numpy()] == [WORD] * 3

    call = Call(hs, data, (1, 3, 1), cap=bound - 1)
    assert call.run(0) == hs.ERR_CAPACITY and untouched(call)
    call = Call(hs, data, (1, 3, 1), ws_short=1)
    assert call.run(0) == hs.ERR_CAPACITY and untouched(call)
    call = Call(hs, data, (1, 3, 1))
    for variant in (4, -1):
        assert call.run(variant) == hs.ERR_ARGUMENT and untouched(call)
    f = hs.lib().hsrle_low_entropy_compress_dev_async
    vp = ctypes.c_void_p
    src, ws, status = call.src.data_ptr(), call.ws.data_ptr(), call.words[1:2].data_ptr()
    args = lambda src, size, at, status: (vp(src), size, 0, vp(call.dst.data_ptr()), call.cap, vp(at), call.ws.numel() - (at - ws), vp(status), vp(torch.cuda.current_stream().cuda_stream))
    assert f(*args(None, n, ws, status)) == hs.ERR_ARGUMENT and untouched(call)              # a null input
    assert f(*args(src, 0, ws, status)) == hs.ERR_ARGUMENT and untouched(call)               # n == 0
    assert hs.low_entropy_workspace_size(0) == 0
    # the words of the workspace take atomics and the status word a word store: odd addresses are refused, not used
    for off in (1, 4, 8):
        assert f(*args(src, n, ws + off, status)) == hs.ERR_ARGUMENT and untouched(call)
    assert f(*args(src, n, ws, status + 2)) == hs.ERR_ARGUMENT and untouched(call)
    with pytest.raises(hs.HsrleError) as e:
        hs.rle8m_compress_async(call.src, 7, call.dst, call.ws[8:], call.words[1:2])
    assert e.value.status == hs.ERR_ARGUMENT and untouched(call)
    assert f(*args(src, n, ws, status)) == hs.OK                                            # and the same call with nothing wrong
    torch.cuda.synchronize()
    assert int(call.words[1].item()) == 0


def test_graph_capture_and_replay(hs, oracle):
    """One encode captured on a side stream (a linear chain of kernels) and replayed on two other inputs of the same length, the workspace refilled with other
    garbage before each replay."""
    import torch

    inputs = [f for f in S.fixtures_a5() if f.data.size == S.A5_SIZE]
    inputs = [inputs[0], inputs[7], inputs[-1]]
    assert inputs[-1].name == "a5.all_equal" and len({f.name for f in inputs}) == 3
    call = Call(hs, inputs[0].data, (1, 3, 1))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert call.run(0, side) == hs.OK                                  # warm-up outside the capture (module load)
    side.synchronize()
    assert call.verdict(oracle.low_entropy_compress(0, inputs[0].bytes)) is None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        assert call.run(0, side) == hs.OK
    for f, garbage in zip(inputs[1:], (0x5A, 0xA5)):
        call.src.copy_(torch.from_numpy(f.data))
        call.refill(garbage)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert call.verdict(oracle.low_entropy_compress(0, f.bytes)) is None, f.name
        assert stats_verdict(hs, call.ws, f.data, 255) is None, f.name


# ---- rle8m: one lane per section (131 072 sections and more) ----

LANE_SECTIONS = S.LANE_SECTIONS


@pytest.fixture(scope="module")
def lane_inputs():
    return S.lane_inputs()


def rle8m_device_verdict(hs, data, sections, want):
    """hsrle_rle8m_compress_dev_async + the decode of what it wrote against the oracle's stream (None: the reference refuses the input)."""
    import torch

    src = to_dev(np.frombuffer(data, dtype=np.uint8), 1)
    cap = hs.rle8m_bounds(sections, len(data))
    buf = torch.full((GUARD + 3 + cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    dst = buf[GUARD + 3 : GUARD + 3 + cap]
    ws = torch.empty(hs.rle8m_workspace_size(len(data), sections), dtype=torch.uint8, device="cuda")
    status = torch.ones(1, dtype=torch.int32, device="cuda")
    hs.rle8m_compress_async(src, sections, dst, ws, status)
    torch.cuda.synchronize()
    del ws
    out = buf.cpu().numpy()
    if not ((out[: GUARD + 3] == 0xEE).all() and (out[GUARD + 3 + cap :] == 0xEE).all()):
        return "a guard was written"
    refused = int(status.item()) != 0
    if want is None or refused:
        return None if (want is None and refused) else f"the oracle {'refuses' if want is None else 'writes a stream'}, status word {int(status.item())}"
    if out[GUARD + 3 : GUARD + 3 + len(want)].tobytes() != want:
        return "stream differs from the oracle's"
    stream = dst[: len(want)].clone()
    info = hs.rle8m_info(stream)
    back = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    hs.rle8m_decompress_async(stream, info, back, status)
    torch.cuda.synchronize()
    return None if int(status.item()) == 0 and torch.equal(back, src) else "decode differs from the input"


def test_the_lane_cases_hold_streams_and_a_refusal(oracle, lane_inputs):
    wants = [oracle.rle8m_compress(sections, data) for data in lane_inputs for sections in LANE_SECTIONS]
    assert sum(w is not None for w in wants) >= 2 and sum(w is None for w in wants) >= 1


@pytest.mark.parametrize("sections", LANE_SECTIONS)
@pytest.mark.parametrize("k", range(3))
def test_rle8m_encode_one_lane_per_section(hs, oracle, lane_inputs, k, sections):
    import torch

    data = lane_inputs[k]
    want = oracle.rle8m_compress(sections, data)
    assert hs.rle8m_compress_dropin(sections, data) == want, "rle8m_compress (host pointers): " + ("the reference refuses this input" if want is None else "stream differs or refused")
    torch.cuda.synchronize()
    assert rle8m_device_verdict(hs, data, sections, want) is None


def test_rle8m_wave_streams_of_the_tie_probes(hs, oracle):
    bad = []
    for f in S.tie_probes_small():
        what = rle8m_device_verdict(hs, f.bytes, 64, oracle.rle8m_compress(64, f.bytes))
        if what:
            bad.append(f"{f.name}: {what}")
    assert not bad, f"{len(bad)} findings, the first: {bad[:8]}"
