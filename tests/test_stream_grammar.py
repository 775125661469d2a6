"""The grammar-written decoder inputs (tests/stream_grammar.py) on the CPU, for all 110 codec ids: the reference decoder -- the oracle's restatement and, where
it was built, the compiled reference -- is the arbiter of what is a legal stream, the parser returns what the writer intended, the fixtures hold every named
form often enough, the encoder-written fixtures of decoder_fixtures hold NONE of the forms called new, and the headers of the W blocks start at every offset.

Everything of a codec is computed once (_facts) and the tests assert their share of it."""
import collections

import pytest

import decoder_fixtures as F
import stream_grammar as G
from hsrle_testlib import CODECS, CODEC_BY_KEY, Reference

B = 4096
# the forms verified by hand against the compiled reference before this module existed, per codec: none of them may hide in G.EXCLUDED
VERIFIED = {
    "wide": ("cnt.u32.small", "rng.u32.small", "hdr.longest", "cnt.min", "term.lit.d", "term.lit.zero", "sym.resent", "op.push.listed", "op.ref.dup", "run.zero",
             "cnt.u16.small", "rng.u16.small", "term.cu32.end", "term.cu32.rd", "term.cu32.ru16", "term.cu32.ru32", "term.cu16.rd", "term.cu16.ru16"),
    "codecs": ("rle8_multi", "rle16_sym", "rle32_byte", "rle64_sym", "rle128_byte", "rle8_packed_multi", "rle16_byte_packed", "rle64_byte_packed", "rle8_3symlut", "rle8_7symlut",
               "rle16_3symlut_sym", "rle24_3symlut_byte", "rle32_7symlut_sym", "rle64_7symlut_byte", "rle8_single", "rle8_packed_single", "rle24_sym_packed", "rle64_sym_packed"),
}

_FACTS = {}


def _reference():
    return Reference() if Reference.available() else None


def _facts(codec):
    if codec.key in _FACTS:
        return _FACTS[codec.key]
    ora, ref, g = F.oracle_instance(), _reference(), G.grammar(codec)
    f = dict(wrong=[], census=collections.Counter(), old=collections.Counter(), residues=set(), straddle64=0, straddle128=0, ratio={}, kinds={}, last_len=None)

    def arbiters(what, stream, want, gr=g):
        try:
            out, forms, headers = G.parse(gr, stream)
        except AssertionError as e:
            f["wrong"].append(f"{what}: the parser refuses the stream ({e})")
            return collections.Counter(), []
        if out != want:
            f["wrong"].append(f"{what}: the parser's output is not the writer's")
        if ora.decompress(codec, stream) != want:
            f["wrong"].append(f"{what}: the oracle's decoder does not give the intended bytes")
        if ref is not None and ref.decompress(codec, stream) != want:
            f["wrong"].append(f"{what}: the compiled reference does not give the intended bytes")
        return forms, headers

    for layout in ("sparse", "dense"):
        fix = G.fixture(codec, layout)
        f["ratio"][layout], f["kinds"][layout], f["last_len"] = fix.ratio, list(fix.kinds), fix.U - (len(fix.kinds) - 1) * B
        f[layout + "_ring"] = F.expected_ring(fix)
        for i, (s, kind) in enumerate(zip(fix.streams, fix.kinds)):
            forms, headers = arbiters(f"{layout} block {i} ({kind})", s, fix.data[i * B : (i + 1) * B].tobytes())
            f["census"] += forms
            if kind == "W":
                for at, n in headers:
                    f["residues"].add(at % 16)
                    f["straddle64"] += at // 64 != (at + n - 1) // 64
                    f["straddle128"] += at // 128 != (at + n - 1) // 128
        for s in F.fixture(codec, layout, B).streams:
            f["old"] += G.parse(g, s)[1]
    monos = [(G.MONO_SIZE, False)] + ([(G.MONO_LONG, True)] if codec.key in G.MONO_LONG_CODECS else [])
    f["mono"] = collections.Counter()
    for size, long_literals in monos:
        s, want = G.mono(codec, size, long_literals)
        if len(want) != size:
            f["wrong"].append(f"monolithic {size}: {len(want)} bytes")
        f["mono"] += arbiters(f"monolithic {size}", s, want)[0]
    if g.stream_symbol and g.kind == "single":
        fix = G.fixture(codec, "dense", modes=(0, 1))
        for i, s in enumerate(fix.streams):
            arbiters(f"modes interleaved, block {i} ({fix.kinds[i]})", s, fix.data[i * B : (i + 1) * B].tobytes(), G.grammar(codec, i % 2))
    if g.has_empty:
        s, want = G.empty_packet_stream(codec)
        f["empty"] = arbiters("empty packets", s, want)[0]["packet.empty"]
    _FACTS[codec.key] = f
    return f


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: c.key)
def test_the_reference_decoder_is_the_arbiter(codec):
    """oracle.decompress and the compiled reference decode every block of both layouts, the monolithic streams, the Single ids' containers of both modes and the
    streams with empty packets to the bytes the writer intended; so does the module's own parser (writer <-> parser round trip)."""
    f = _facts(codec)
    assert not f["wrong"], f"{codec.key}: {len(f['wrong'])} streams, the first: {f['wrong'][:3]}"
    if G.grammar(codec).has_empty:
        assert f["empty"] >= 3, "the stream with empty packets has some"


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: c.key)
def test_every_named_form_occurs(codec):
    """The census of the codec's two containers: every new form at least MIN_PACKET_FORMS (terminator forms: MIN_TERM_FORMS) times; no packet without a byte
    (those come in a stream of their own); the monolithic streams hold the packet forms too."""
    f, g = _facts(codec), G.grammar(codec)
    for form in G.new_forms(g):
        need = G.MIN_TERM_FORMS if form.startswith("term.") else G.MIN_PACKET_FORMS
        assert f["census"][form] >= need, f"{codec.key}: {form} occurs {f['census'][form]} times, {need} wanted"
        if not form.startswith("term."):
            assert f["mono"][form] >= 3, f"{codec.key}: the monolithic streams hold {form} {f['mono'][form]} times"
    assert f["census"]["packet.empty"] == 0 and f["mono"]["packet.empty"] == 0


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: c.key)
def test_the_encoders_write_none_of_the_new_forms(codec):
    """The gap, proven: the same census over the encoder-written containers of decoder_fixtures (4 KiB, both layouts) reports zero for every form called new."""
    f, g = _facts(codec), G.grammar(codec)
    assert sum(f["old"].values()) > 500, "the census read the old fixtures"
    found = {form: f["old"][form] for form in G.new_forms(g) if f["old"][form]}
    assert not found, f"{codec.key}: the encoders do write {found}"


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: c.key)
def test_layouts_and_header_placement(codec):
    """Both containers have the default shape (three waves, the last block partial and off a 16-byte boundary), every full wave its mixture, the ratios lie on the
    two sides of the ring thresholds; the headers of the W blocks start at every residue mod 16, some straddle a multiple of 64 and of 128 stream bytes."""
    f = _facts(codec)
    assert f["ratio"]["sparse"] <= 0.18 and f["ratio"]["dense"] >= 0.40, f["ratio"]
    assert f["sparse_ring"] == (64 if codec.S <= 4 else 128) and f["dense_ring"] == 128
    assert f["last_len"] == B // 2 + 5 and f["last_len"] % 16 != 0
    for layout in ("sparse", "dense"):
        kinds = f["kinds"][layout]
        assert len(kinds) == 3 * G.WAVE
        for w in range(3):
            assert collections.Counter(kinds[w * G.WAVE : (w + 1) * G.WAVE]) == dict(G.LAYOUTS[layout])
    assert f["residues"] == set(range(16)), f"{codec.key}: header starts of the W blocks miss the residues {set(range(16)) - f['residues']}"
    assert f["straddle64"] >= 1 and f["straddle128"] >= 1


def test_exclusions_are_the_references_own():
    """Every entry of G.EXCLUDED is a form the compiled reference refuses or decodes differently -- and none of the forms verified by hand for the codecs named in
    the issue is excluded (so a writer bug cannot hide there)."""
    families = {G.grammar(CODEC_BY_KEY[k]).family for k in VERIFIED["codecs"]}
    for (family, form), reason in G.EXCLUDED.items():
        assert reason and not (family in families and form in VERIFIED["wide"]), f"{family} {form} was verified against the reference"
    assert all(form not in forms for (fam, form) in G.EXCLUDED for forms in [G.NEW_FORMS.get(fam, ())]), "an excluded form is not generated"


def test_the_fixture_is_deterministic():
    codec = CODEC_BY_KEY["rle24_3symlut_byte_short"]
    a = G.fixture(codec, "dense")
    G._CACHE.clear()
    b = G.fixture(codec, "dense")
    assert a.container == b.container and a.kinds == b.kinds
    assert G.mono(codec) == G.mono(codec)
