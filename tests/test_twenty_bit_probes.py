"""The reference's 20-bit range rule (a range or a stored count above 0xFFFFF costs 4, not 2: src/rleX_Xsl.h:130, src/rleX_Xsl_short.h:197) on the CPU:
the oracle -- and the compiled reference where it is built -- decide every probe of tests/twenty_bit_probes.py as tests/golden/twenty_bit_probes.json
records it (minted from the compiled reference by tests/golden/make_twenty_bit_golden.py), and the golden file keeps the probes that flip."""
import numpy as np
import pytest

import twenty_bit_probes as P
from hsrle_testlib import CODEC_BY_KEY

KEYS = [c.key for c in P.RULE_CODECS]
FLIPPING_CODECS_MIN = 58          # what the mint found when the file was first written: a regenerated file with fewer makes the GPU suite vacuous
FLIPPING_CHUNK_SHORT_MIN = 16     # ... of the 22 Short codecs whose monolithic chunks go to the windowed encoder (hsrle_codecs.h: chunk_mode)


@pytest.fixture(scope="module")
def golden():
    return P.load_golden()


def _inputs(codec, g):
    """(what, input, golden entry) of every recorded stream of one codec: each probe alone, the count probe, the monolithic input."""
    probes = P.plan(codec, {"codecs": {codec.key: g}})
    for p, e in zip(probes, g["probes"]):
        yield f"{p.variant} count {p.count} gap {p.gap}", P.build_probe(codec.S, p.variant, p.count, p.gap, p.sym_index), e
    yield "count probe", P.build_count_probe(codec), g["count_probe"]
    data, used = P.mono_input(codec, probes)
    assert used == g["mono"]["probes"] and data.size == g["mono"]["size"] <= P.MONO_MAX
    yield "monolithic input", data, g["mono"]


def _check_codec(enc, codec, g):
    for what, data, e in _inputs(codec, g):
        stream = enc.compress(codec, data.tobytes())
        assert stream is not None and (len(stream), P.sha(stream)) == (e["length"], e["sha256"]), f"{codec.key} {what}"
    blocks = P.container_input(codec, P.plan(codec, {"codecs": {codec.key: g}})).reshape(-1, P.BLOCK)
    streams = [enc.compress(codec, b.tobytes()) for b in blocks]
    assert [len(s) for s in streams] == g["container"]["lengths"] and P.sha(b"".join(streams)) == g["container"]["sha256"], f"{codec.key} container blocks"


@pytest.mark.parametrize("key", KEYS)
def test_oracle_decides_as_the_golden_file(oracle, golden, key):
    codec, g = CODEC_BY_KEY[key], golden["codecs"][key]
    _check_codec(oracle, codec, g)
    for p, e in zip(P.plan(codec, golden), g["probes"]):            # `stored` is what the stream says
        data = P.build_probe(codec.S, p.variant, p.count, p.gap, p.sym_index)
        runs = oracle.run_packets(codec, oracle.compress(codec, data.tobytes()), data.size)
        assert runs == e["run_packets"] and runs - int(e["stored"]) in (0, 1), f"{key} {p.key()}"
    assert P.stored_count(codec, g["count_probe"]["count"]) > P.T and g["count_probe"]["stored"]


@pytest.mark.parametrize("key", KEYS)
def test_reference_decides_as_the_golden_file(reference, golden, key):
    _check_codec(reference, CODEC_BY_KEY[key], golden["codecs"][key])


@pytest.mark.parametrize("key", KEYS)
def test_filler_holds_no_run(reference, oracle, key):
    """The reference's stream of T + 64 filler bytes is the input plus a header and a terminator (at most 25 bytes for every codec), no run packet."""
    codec = CODEC_BY_KEY[key]
    data = P.filler(P.T + 64).tobytes()
    stream = reference.compress(codec, data)
    assert len(data) < len(stream) <= len(data) + 25
    assert reference.decompress(codec, stream, len(data)) == data and oracle.run_packets(codec, stream, len(data)) == 0
    assert oracle.compress(codec, data) == stream


def test_filler_has_no_equal_bytes_nearby():
    f = P.filler(1 << 17, 5).astype(np.int16)
    for d in range(1, 17):
        assert not (f[d:] == f[:-d]).any(), d
    step = (f[1:] - f[:-1]) & 0xFF
    assert not (step == 1).any()                                       # no two bytes of a probe symbol (A1 A2 ..) in a row


def test_probe_plan_follows_the_recorded_flips(golden):
    """The golden file's probes are probe_list() of its flips: four per flipping variant, two elsewhere, pairs that differ only in the gap."""
    for key in KEYS:
        codec, g = CODEC_BY_KEY[key], golden["codecs"][key]
        want = P.probe_list(codec.S, g["flips"])
        assert [p.key() for p in want] == [p.key() for p in P.plan(codec, golden)], key
        for v in P.VARIANTS:
            assert all(c in P.count_candidates(codec.S) for c in g["flips"][v]), key


def test_the_suite_is_not_vacuous(golden):
    """At least the 58 codecs the mint named have a probe pair (same count, same variant) whose `stored` differs across the gap -- stored at range T,
    not stored at T + 1 -- and 16 of the 22 chunk-mode Short codecs are among them."""
    flipping = []
    for key in KEYS:
        probes = golden["codecs"][key]["probes"]
        by = {(e["variant"], e["count"], e["gap"]): i for i, e in enumerate(probes)}
        pairs = [(i, by[(v, c, P.GAPS[1])]) for (v, c, gap), i in by.items() if gap == P.GAPS[0] and (v, c, P.GAPS[1]) in by]
        pairs = [(i, j) for i, j in pairs if probes[i]["stored"] and not probes[j]["stored"]]
        if pairs:
            flipping.append(key)
            mono = golden["codecs"][key]["mono"]["probes"]
            assert any(i in mono and j in mono for i, j in pairs), f"{key}: the monolithic input has no flipping pair"
    assert sorted(flipping) == golden["flipping"]
    assert len(flipping) >= FLIPPING_CODECS_MIN
    chunk_short = [k for k in KEYS if P.is_chunk_mode_short(CODEC_BY_KEY[k])]
    assert len(chunk_short) == 22
    assert len([k for k in flipping if k in chunk_short]) >= FLIPPING_CHUNK_SHORT_MIN
