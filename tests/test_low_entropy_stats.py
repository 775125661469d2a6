"""The model of the low-entropy encoders' statistics and tables (tests/low_entropy_stats.py) against the oracle -- and, where it was built, the compiled
reference -- on the inputs that sit on the encoders' thresholds: for every fixture the model's header is the header of the oracle's stream, for the four
unsectioned variants and for rle8m with 1 and 7 sections; the counts are those of a plain restatement of the reference's loop; and every probe is
SENSITIVE: one step of the probed count in the losing direction changes the tables (a probe for which it does not would prove nothing on the GPU)."""
import ctypes

import numpy as np
import pytest

import low_entropy_stats as S
from hsrle_testlib import Reference


class CompressInfo(ctypes.Structure):
    _fields_ = [("rle", ctypes.c_uint8 * 256), ("symbolsByProb", ctypes.c_uint8 * 256), ("symbolCount", ctypes.c_uint8)]


def oracle_headers(oracle, data):
    """The info bytes the oracle writes for `data`: [variant 0 .. 3 of the unsectioned forms, rle8m with 1 section, with 7].  Read from the output buffer, so
    also where the oracle then gives the stream up (a section that outgrows the room left: the header is written first)."""
    L = oracle.lib
    L.hso_low_entropy_compress.restype = ctypes.c_uint32
    L.hso_low_entropy_compress.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    L.hso_rle8m_compress.restype = ctypes.c_uint32
    L.hso_rle8m_compress.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    n = data.size
    out = np.zeros(3 * n + 1024, dtype=np.uint8)                     # (a stream can be twice its input, and the oracle writes it like the reference)
    heads = []

    def info(at):
        listed = int(out[at + 32]) or 255
        return out[at : at + 33 + listed].tobytes()

    for variant in range(4):
        assert L.hso_low_entropy_compress(variant, data.ctypes.data, n, out.ctypes.data, n + 297) > 0
        heads.append(info(8))
    for sections in (1, 7):
        if n >= sections:
            L.hso_rle8m_compress(sections, data.ctypes.data, n, out.ctypes.data, n + 289 + 4 * (sections + 2))
            assert int(out[4:8].view("<u4")[0]) == n and int(out[8:12].view("<u4")[0]) == sections
            heads.append(info(12 + 4 * (sections - 1)))
    return heads


def model_headers(data):
    h = [S.model_header(data, 32 if v & 1 else 255, v >> 1) for v in range(4)]
    return h + [h[0]] * (2 if data.size >= 7 else 1)


def plain_stats(data, max_len):
    """The reference's loop as it stands (hsrle_oracle.c:1385-1405), the start-up wrap of pcount[0] included."""
    prob, pcount = [0] * 256, [0] * 256
    last, count = 0, 0
    if data[0] != last:
        pcount[last] = 0xFFFFFFFF
    for b in data:
        if b == last:
            count += 1
        else:
            prob[last] += count
            pcount[last] = (pcount[last] + count // max_len + 1) & 0xFFFFFFFF
            count, last = 1, b
    prob[last] += count
    pcount[last] = (pcount[last] + 1) & 0xFFFFFFFF
    return prob, pcount


@pytest.fixture(scope="module")
def small():
    return S.fixtures_small()


def check_headers(oracle, fixtures):
    bad = [f.name for f in fixtures if model_headers(f.data) != oracle_headers(oracle, f.data)]
    assert not bad, f"the model's header is not the oracle's: {bad[:10]} ({len(bad)} of {len(fixtures)})"


def test_the_fixtures_are_what_they_claim():
    a1, a2, a4, a5 = S.fixtures_a1(), S.fixtures_a2(), S.fixtures_a4(), S.fixtures_a5()
    assert len(a1) >= 200 and len(a2) >= 600 and len(S.tie_probes_small()) >= 120
    assert len({f.name for f in a1 + a2 + a4 + a5}) == len(a1 + a2 + a4 + a5)
    assert all(f.data.size == S.SMALL for f in S.tie_probes_small())
    used = [int((S.stats(f.data, 255)[1] > 0).sum()) for f in a4]
    assert used[:4] == [256, 256, 255, 255] and used[4:] == [1, 1]
    flags, order, count = S.tables(*S.stats(a4[0].data, 255), 0)
    assert count == 0 and len(S.header_bytes(flags, order, count)) == 33 + 255          # 256 symbols in use: the count byte is 0, 255 are listed
    assert sum(f.data.size == S.A5_SIZE for f in a5) >= 49 and a5[-1].name == "a5.all_equal"
    assert [f.data.size for f in S.fixtures_a3_mid()] == [S.A3_MID] * 5 and [f.data.size for f in S.fixtures_a3_carry()] == [S.A3_CARRY] * 2


def test_every_probe_is_sensitive(small):
    """The condition of the probes: one step of the probed count, in the direction that loses, changes tables(...)."""
    probes = [f for f in small if f.moves]
    assert len(probes) >= 800
    for f in probes:
        prob, pcount = S.stats(f.data, f.max_len)
        for only_max, which, sym, delta in f.moves:
            was = S.tables(prob, pcount, only_max)
            now = S.tables(*S.moved(prob, pcount, which, sym, delta), only_max)
            assert any(not np.array_equal(a, b) for a, b in zip(was, now)), f"{f.name}: {which}[{sym}] {delta:+d} (only_max {only_max}) changes nothing"


def test_the_model_counts_like_the_reference_loop(small):
    for f in small[::9] + S.fixtures_a4() + S.fixtures_a5()[::7]:
        for max_len in (255, 32):
            prob, pcount = S.stats(f.data, max_len)
            assert (prob.tolist(), pcount.tolist()) == plain_stats(f.data.tolist(), max_len), f"{f.name}, max_len {max_len}"


def test_model_header_is_the_oracle_header_small(oracle, small):
    check_headers(oracle, small)


def test_model_header_is_the_oracle_header_cut_edges(oracle):
    check_headers(oracle, S.fixtures_a5())


def test_model_header_is_the_oracle_header_scan_edges(oracle):
    check_headers(oracle, S.fixtures_a3_mid() + S.fixtures_a3_carry())


def test_model_header_is_the_oracle_header_second_piece_per_wave(oracle):
    f = S.fixture_a3_big()
    assert f.data.size == S.A3_BIG and 0.01 < float((f.data != 0).mean()) < 0.03
    for m, x, y in ((255, 200, 201), (32, 211, 210)):
        pcount = S.stats(f.data, m)[1]
        assert pcount[x] == pcount[y] > 16                                            # the tie probes at piece 32768
    check_headers(oracle, [f])


def test_the_lane_per_section_cases_hold_streams_and_a_refusal(oracle):
    """The condition of the rle8m cases with 131 072 sections and more: the oracle writes a stream for at least two of them and refuses at least one."""
    wants = [oracle.rle8m_compress(sections, data) for data in S.lane_inputs() for sections in S.LANE_SECTIONS]
    assert sum(w is not None for w in wants) >= 2 and sum(w is None for w in wants) >= 1


def test_model_tables_are_the_compiled_reference_structs(small):
    """rle8_low_entropy_get_compress_info[_only_max_frequency] of the reference's own code, struct for struct (they count with max_len 255)."""
    if not Reference.available():
        pytest.skip("oracle/_ref/libhsrle_ref.so not built (needs the reference's sources)")
    ref = Reference().lib
    getters = []
    for name in ("rle8_low_entropy_get_compress_info", "rle8_low_entropy_get_compress_info_only_max_frequency"):
        g = getattr(ref, name)
        g.restype = ctypes.c_bool
        g.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(CompressInfo)]
        getters.append(g)
    fixtures = small + S.fixtures_a5() + S.fixtures_a3_mid() + S.fixtures_a3_carry() + [S.fixture_a3_big()]
    for f in fixtures:
        prob, pcount = S.stats(f.data, 255)
        for only_max, getter in enumerate(getters):
            info = CompressInfo()
            assert getter(f.data.ctypes.data, f.data.size, ctypes.byref(info))
            flags, order, count = S.tables(prob, pcount, only_max)
            assert bytes(info) == flags.tobytes() + order.tobytes() + bytes([count]), f"{f.name}, only_max {only_max}"
