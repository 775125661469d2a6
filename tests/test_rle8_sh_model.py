"""The sequential models of rle8_sh (rle8_sh_testlib.py) against the compiled reference (skipped where it is absent) and against the stored vectors
minted from it (tests/golden/rle8_sh/vectors.json).  The GPU tests compare the library with these models."""
import json
import random

import pytest

import rle8_sh_testlib as T

needs_reference = pytest.mark.skipif(not T.Rle8ShReference.available(), reason="oracle/_ref/libhsrle_ref.so is not built")

INPUTS = T.input_set()
GRAMMAR = T.grammar_streams()


@pytest.fixture(scope="module")
def ref():
    return T.Rle8ShReference()


def golden():
    with open(T.GOLDEN) as f:
        return json.load(f)["vectors"]


@needs_reference
def test_bounds_are_the_references(ref):
    for n in (0, 1, 1000, 1 << 30):
        assert ref.bounds(n) == n + 13


@needs_reference
@pytest.mark.parametrize("name", list(INPUTS))
def test_encoder_models_against_reference(ref, name):
    data = INPUTS[name]
    theirs = ref.compress(data)
    by_run, items = T.model_compress(data)
    by_byte, items2 = T.model_compress_bytewise(data)
    assert by_byte == theirs, "the byte loop restated differs from the reference"
    assert by_run == theirs and items == items2, "the run-level loop differs from the reference"
    assert ref.decompress(theirs, len(data)) == (len(data), data)


@needs_reference
def test_encoder_model_against_reference_on_random_inputs(ref):
    rng = random.Random(2)
    for t in range(300):
        data = T.geometric_runs(rng.randrange(1, 3000), rng.choice((1, 2, 3, 4, 8, 256)), t, mean=rng.choice((2, 6, 12, 20)))
        assert T.model_compress(data)[0] == ref.compress(data), t


def test_encoder_models_against_stored_reference_streams():
    vectors = golden()
    assert len(vectors) >= 90
    for v in vectors:
        data, stream = bytes.fromhex(v["input"]), bytes.fromhex(v["stream"])
        assert INPUTS[v["name"]] == data, v["name"]
        assert T.model_compress(data)[0] == stream, v["name"]
        assert T.model_compress_bytewise(data)[0] == stream, v["name"]


def test_the_decision_kernels_shortcut_changes_nothing():
    """k_she_decide takes whole words of short runs at once (model_compress_words restates it): same stream, same items, and it IS taken."""
    rng = random.Random(6)
    taken = 0
    extra = [rng.randbytes(5000), T.geometric_runs(6000, 256, 1, mean=2), T.geometric_runs(6000, 8, 2, mean=3), T.raw_blocks_between_changes(5000)]
    for data in list(INPUTS.values()) + extra:
        by_run, items = T.model_compress(data)
        by_word, items2, cut = T.model_compress_words(data)
        assert by_word == by_run and items2 == items
        taken += cut
    assert taken > 200


def test_decoder_model_on_stored_reference_streams():
    for v in golden():
        assert T.model_decompress(bytes.fromhex(v["stream"])) == bytes.fromhex(v["input"]), v["name"]


@needs_reference
@pytest.mark.parametrize("name", list(GRAMMAR))
def test_decoder_model_against_reference_on_grammar_streams(ref, name):
    """Streams no encoder writes: literals that promote behind S / T, FILL large counts through the wrap, a gap, every token in front of the end."""
    stream = GRAMMAR[name]
    want = T.model_decompress(stream)
    assert want is not None
    assert ref.decompress(stream, len(want)) == (len(want), want)


def test_writer_and_parser_are_inverse():
    for name, stream in GRAMMAR.items():
        n, tokens, out = T.parse_stream(stream)
        gap = 5 if name == "gap_between_body_and_bits" else 0
        assert T.write_stream(n, tokens, gap=gap) == stream, name
        assert len(out) == n


def test_wrapped_fill_counts():
    for c in (0, 9, 10, 13):
        assert T.wrapped(c) >= 0xFFFFFFF2
        stream = T.write_stream(c + 1, [("FILLL", T.wrapped(c), 0x42), ("Z",), ("END",)])
        assert T.model_decompress(stream) == b"\x42" * (c + 1)


def test_malformed_streams_are_malformed_for_the_model():
    good, bad = T.malformed_streams()
    assert T.model_decompress(good) is not None
    for name, (n, stream) in bad.items():
        if name != "header_size_is_not_the_output_size":
            assert T.model_decompress(stream) is None, name


def test_capacity_bound_on_the_models_streams():
    cap = lambda n: n + n // 221 + 21  # noqa: E731  (hsrle_rle8_sh_capacity, include/hsrle.h)
    rng = random.Random(3)
    for data in list(INPUTS.values()) + [rng.randbytes(n) for n in (1, 7, 8, 300, 5000)] + [T.short_coded_stretches(4000), T.raw_blocks_between_changes(273 * 40 + 5),
                                                                                                  T.marginal_encoded_spans(5000), T.marginal_encoded_spans(20000)]:
        assert len(T.model_compress(data)[0]) <= cap(len(data))
    # the worst case per byte: 1.875 bytes per block of 416 and nothing saved inside; far past the constant slack, and within 1 % of n / 221.9
    worst = T.marginal_encoded_spans(20000)
    growth = len(T.model_compress(worst)[0]) - len(worst)
    assert 0.99 * len(worst) * 1.875 / 416 < growth <= len(worst) // 221 + 21
    grown = T.raw_blocks_between_changes(273 * 40)
    # 40 raw COPY large (7 bits + 4 bytes each), 39 changes of R (7 bits + 5 bytes for 10 bytes: the last run has no successor and stays in its
    # block), the terminator (7 bits + 4), the header (8): 80 tokens of 7 bits = 70 bytes, body n - 390 + 160 + 195 + 4
    assert len(T.model_compress(grown)[0]) == len(grown) + 47
