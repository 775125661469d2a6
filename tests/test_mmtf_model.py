"""The mmtf / bitmmtf model without a GPU: the sequential definition (tests/mmtf_testlib.py) against stored vectors of the compiled reference
(tests/golden/mmtf/, minted by tests/golden/make_mmtf_golden.py) and against the compiled reference itself where it is present, and the segment
algebra of the kernels (tools/mmtf_segment_model.py: state per segment, scan of the compositions, run from the true start list) against the
sequential definition."""
import json
import os
import sys

import pytest

import mmtf_testlib as mt

sys.path.insert(0, os.path.join(mt.REPO, "tools"))
import mmtf_segment_model as seg  # noqa: E402


def golden():
    with open(os.path.join(mt.GOLDEN_DIR, "vectors.json")) as f:
        return json.load(f)["vectors"]


@pytest.mark.parametrize("transform", mt.TRANSFORMS)
@pytest.mark.parametrize("decode", (0, 1))
def test_model_equals_stored_reference_vectors(transform, decode):
    vectors = golden()
    assert len(vectors) >= 5
    for v in vectors:
        data = bytes.fromhex(v["input"])
        assert mt.model(transform, decode, data).hex() == v[mt.function_name(transform, decode)], v["name"]


@pytest.fixture(scope="module")
def ref():
    if not mt.MmtfReference.available():
        pytest.skip("oracle/_ref/libhsrle_ref.so not built (needs the reference's sources)")
    return mt.MmtfReference()


@pytest.mark.parametrize("transform", mt.TRANSFORMS)
@pytest.mark.parametrize("misalign", (0, 1))
def test_model_equals_compiled_reference(ref, transform, misalign):
    W = mt.WIDTH[transform]
    for n in (0, 1, W - 1, W, W + 1, 64 * W + 5, 2003):
        for alphabet in (1, 2, 5, 40, 256):
            data = mt.random_bytes(n, alphabet, 17 + misalign)
            for decode in (0, 1):
                rc, out = ref.run(transform, decode, data, misalign=misalign)
                assert rc == n
                assert out == mt.model(transform, decode, data), (n, alphabet, decode)


def test_reference_return_values(ref):
    assert ref.bounds("mmtf_bounds", 1000) == 1000 and ref.bounds("bitmmtf_bounds", 1000) == 1000
    for t in mt.TRANSFORMS:
        for decode in (0, 1):
            assert ref.run(t, decode, bytes(32), out_size=31)[0] == 0
            assert ref.run(t, decode, b"")[0] == 0


SEG_SIZES = lambda W: (0, 1, W - 1, W, W + 1, 64 * W + 5, 20003)  # noqa: E731


@pytest.fixture(scope="module")
def seg_inputs():
    """inputs and their sequential transforms, computed once"""
    cases = {}
    for W in (16, 32):
        inputs = []
        for n in SEG_SIZES(W):
            for alphabet in (1, 2, 5, 256):
                inputs.append(mt.random_bytes(n, alphabet, 29))
        inputs.append(mt.every_symbol_per_column(20003, W))
        inputs.append(mt.every_symbol_per_column(64 * W + 5, W))
        cases[W] = [(d, mt.mmtf_enc(d, W), mt.mmtf_dec(d, W)) for d in inputs]
    return cases


@pytest.mark.parametrize("W", (16, 32))
@pytest.mark.parametrize("segment_rows", (1, 2, 7, 64))
def test_segment_algebra_equals_sequential(seg_inputs, W, segment_rows):
    for data, enc, dec in seg_inputs[W]:
        assert seg.segment_encode(data, W, segment_rows) == enc, (len(data), "encode")
        assert seg.segment_decode(data, W, segment_rows) == dec, (len(data), "decode")


def test_segment_model_states():
    """the closed forms one by one: P composes, (F, K) rebuilds the list, K counts distinct symbols"""
    data = mt.random_bytes(500, 40, 31)
    start = list(range(255, -1, -1))
    l = list(start)
    for k in data:
        l.insert(0, l.pop(k))
    assert seg.compose_decode(start, seg.pass_a_decode(data)) == l
    f, k = seg.pass_a_encode(data)
    assert k == len(set(data))
    l = list(start)
    for x in data:
        l.insert(0, l.pop(l.index(x)))
    assert seg.compose_encode(start, f, k) == l
