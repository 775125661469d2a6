"""The low-entropy streams written from the grammar (tests/low_entropy_grammar.py) on the CPU: the sequential model, the bounds-checked parser and
the oracle's decoders agree on every fixture that tests/test_gpu_low_entropy_grammar.py hands to the GPU; the fixtures hold every form the grammar
names; the oracle refuses every malformed one.  Where the compiled reference is present it is held against the same bytes on the class of streams it
agrees on, and its three departures are pinned.

The reference's decoders check no bounds, so they only ever see well-formed streams, with room behind both buffers, in a child process with an
interpreter of its own (this file run as a program): if one of them ends that process the test says so instead of taking the suite with it."""
import ctypes
import os
import pickle
import random
import shutil
import struct
import subprocess
import sys
from collections import Counter

import pytest

import low_entropy_grammar as G

PAD = 4096


def all_well_formed():
    """(name, stream, sectioned) of every well-formed fixture"""
    for name, s in G.le_fixtures().items():
        yield "le." + name, s, False
    for name, (s, _) in G.le_limit_fixtures().items():
        yield "le." + name, s, False
    for name, s in G.rle8m_fixtures().items():
        yield "rle8m." + name, s, True
    yield "rle8m.lane_small", G.lane_small(), True


_PARSED = {}


def parsed(name, stream, sectioned):
    if name not in _PARSED:
        _PARSED[name] = G.parse(stream, sectioned)
    return _PARSED[name]


def oracle_decode(oracle, stream, sectioned, in_size=None, out_cap=None):
    """(return value, the whole output buffer: 0xEE where nothing was written)"""
    f = oracle.lib.hso_rle8m_decompress if sectioned else oracle.lib.hso_low_entropy_decompress
    f.restype = ctypes.c_uint32
    out_size = struct.unpack_from("<I", stream, 4)[0] if len(stream) >= 8 else 0
    cap = out_size if out_cap is None else out_cap
    out = ctypes.create_string_buffer(b"\xEE" * (cap + PAD), cap + PAD)
    got = f(bytes(stream), ctypes.c_uint32(len(stream) if in_size is None else in_size), out, ctypes.c_uint32(cap))
    return got, out.raw


def test_tables_follow_the_references_rule():
    assert G.tables((), [7, 3]) == [2, 3, 4, 1, 5, 6, 7, 0] + list(range(8, 256))
    t = G.tables((), [7, 3, 7])                                          # the last listing wins; position 0 has no code; the tail starts at 3
    assert (t[7], t[3], t[0], t[255]) == (2, 1, 3, (3 + 253) & 0xFF) and G.codes_of(t)[0] == [255]
    t = G.tables((), list(range(255)), n_byte=0)                         # a stored 0 means 255 listed symbols
    assert t == list(range(256))
    t = G.tables((), [9] * 255)                                          # modulo 256: count 254 + 2 = 0
    assert t[9] == 254 and t[0] == 255 and t[1] == 0 and t[2] == 1


def test_model_parser_and_oracle_agree_on_every_fixture(oracle):
    n = 0
    for name, stream, sectioned in all_well_formed():
        want = G.model(stream, sectioned)
        out, _ = parsed(name, stream, sectioned)
        assert out == want, f"{name}: the parser and the model differ"
        assert len(want) == struct.unpack_from("<I", stream, 4)[0], name
        got, buf = oracle_decode(oracle, stream, sectioned)
        assert got == len(want) and buf[: len(want)] == want, f"{name}: the oracle and the model differ"
        assert buf[len(want) :] == b"\xEE" * PAD, f"{name}: the oracle wrote behind the output"
        n += 1
    assert n > 90
    stream, want = G.lane_stream()                                      # the tiled stream: the oracle reads all of it
    got, buf = oracle_decode(oracle, stream, True)
    assert got == len(want) and buf[: len(want)] == want


def test_the_fixtures_hold_every_form():
    total = Counter()
    for name, stream, sectioned in all_well_formed():
        total += parsed(name, stream, sectioned)[1]
    missing = [f for f in G.FORMS if total[f] == 0]
    assert not missing, f"no fixture holds {missing}"
    # the named header fixtures hold the form they are named after
    for name, (h, toks) in G.header_forms().items():
        if name in G.FORMS:
            assert parsed("le.form." + name, G.le_fixtures()["form." + name], False)[1][name] > 0, name


def test_the_edge_fixtures_put_the_bytes_where_they_say():
    """stream byte dataStart + edge - 1 of the piece / window fixtures is what the placement names"""
    for h in (G.HF, G.HP):
        for unit in (G.PIECE, G.WINDOW):
            body = bytes(G.edge_body(h, unit))
            step = unit if unit >= 512 else unit * 5
            for k, (name, front, _) in enumerate(G.placements(h)):
                E = step * (k + 1)
                last = body[E - 1]
                if name == "plain":
                    assert last not in h.flags and body[E - 2] not in h.flags
                elif name.startswith("sym.code"):
                    c = int(name[8:])
                    assert last == G.F2 and body[E - 2] not in h.flags and h.count_of[body[E]] == c and (body[E] in h.flags) == (h is G.HF)
                elif name.startswith("code"):
                    assert body[E - 2] == G.F3 and body[E - 3] not in h.flags and (last in h.flags) == name.endswith("flagged_value")
                else:
                    assert all(b in h.flags for b in body[E - front : E]) and body[E - front - 1] not in h.flags, name
    for length, attempts in ((G.CARRY_LIMIT - 1, 1), (G.CARRY_LIMIT, 2), (G.CARRY_LIMIT + 1, 2)):
        body, E = bytes(G.limit_body(length)), 5 * G.PIECE
        assert all(b in G.HF.flags for b in body[E - length : E]) and body[E - length - 1] not in G.HF.flags and body[E + 1] not in G.HF.flags
        assert G.le_limit_fixtures()[f"limit.{length}"][1] == attempts
    assert all(b in G.HF.flags for b in G.one_stretch_body())
    # the ladder: every packet length at every output offset modulo 16
    seen, o, body = set(), 0, bytes(G.ladder_body())
    i = 0
    while i < len(body):
        if body[i] == G.F0:
            seen.add((1 + body[i + 1], o % 16))
            o += 1 + body[i + 1]
            i += 2
        else:
            o += 1
            i += 1
    assert seen == {(length, ph) for length in range(1, 256) for ph in range(16)}
    # the lane patterns: every count at every phase of the accumulator
    seen = set()
    for p in G.lane_patterns():
        i = o = 0
        while i < len(p):
            if p[i] == G.F0:
                seen.add((p[i + 1], (o + 1) % 16))
                o += 1 + p[i + 1]
                i += 2
            else:
                o += 1
                i += 1
    assert seen >= {(c, ph) for c in G.LANE_COUNTS for ph in range(16)}
    assert len(G.lane_patterns()) == G.LANE_PATTERNS and max(len(p) for p in G.lane_patterns()) > 2 * 32
    assert any(G.F0 not in p for p in G.lane_patterns())


def test_malformed_streams_are_refused_by_parser_and_oracle(oracle):
    rules = set()
    for sectioned, fx in ((False, G.le_malformed()), (True, G.rle8m_malformed())):
        for name, (stream, rule) in fx.items():
            with pytest.raises(G.Malformed) as e:
                G.parse(stream, sectioned)
            assert e.value.rule == rule, name
            rules.add((sectioned, rule))
            out_size = struct.unpack_from("<I", stream, 4)[0]
            got, buf = oracle_decode(oracle, stream, sectioned)
            assert got == 0, f"{name}: the oracle accepts it"
            assert buf[out_size:] == b"\xEE" * PAD, f"{name}: the oracle wrote behind the output"
    header = {"size.above_buffer", "info.past_stream", "list.past_stream"}
    body = {"out.over", "out.under", "count.past_share", "flagged.last_byte"}
    assert {r for s, r in rules if not s} == header | body
    assert {r for s, r in rules if s} == header | body | {"sections.zero", "section.end_below_data", "section.end_below_begin", "section.end_above_size"}


def test_random_streams_from_the_grammar(oracle):
    """lists that are short, permuted, hold duplicates or are stored as 0; 1 .. 256 flags; every count: model == parser == oracle"""
    rng = random.Random(600)
    for trial in range(150):
        nflags = rng.choice([1, 1, 2, 3, 8, 64, 255, 256])
        flags = rng.sample(range(256), nflags)
        kind = rng.randrange(4)
        n_byte = None
        if kind == 0:
            listed = rng.sample(range(256), rng.randrange(1, 256))
        elif kind == 1:
            listed = [rng.randrange(256) for _ in range(rng.randrange(1, 256))]      # duplicates
        elif kind == 2:
            listed, n_byte = rng.sample(range(256), 255), 0
        else:
            listed = [rng.choice(flags + [rng.randrange(256)]) for _ in range(255)]
        h = G.Header(flags, listed, n_byte)
        toks = G._random_tokens(h, rng, rng.randrange(1, 200), list(range(255)))
        for sectioned, stream in ((False, G.write_le(flags, listed, toks, n_byte)), (True, G.write_rle8m(flags, listed, [toks] * rng.choice([1, 2, 5]), n_byte))):
            want = G.model(stream, sectioned)
            assert G.parse(stream, sectioned)[0] == want
            got, buf = oracle_decode(oracle, stream, sectioned)
            assert got == len(want) and buf[: len(want)] == want, trial


# ------------------------------------------------------------------------------------------------------------------
# the compiled reference


def ref_decode(lib, fname, stream, in_size=None, in_pad=PAD):
    """(return value, output buffer of out_size + PAD bytes, 0xEE where nothing was written)"""
    f = getattr(lib, fname)
    f.restype = ctypes.c_uint32
    out_size = struct.unpack_from("<I", stream, 4)[0]
    src = ctypes.create_string_buffer(bytes(stream) + b"\x55" * in_pad, len(stream) + in_pad)
    out = ctypes.create_string_buffer(b"\xEE" * (out_size + PAD), out_size + PAD)
    got = f(src, ctypes.c_uint32(len(stream) if in_size is None else in_size), out, ctypes.c_uint32(out_size))
    return got, out.raw


# what the child process runs (JOBS[name](Reference(), *args)); nothing here is called in the test process


def job_agree(reference, cases):
    bad = []
    for level in ((0, 99) if reference.has_avx2 else (99,)):
        reference.set_max_simd(level)
        for name, stream, sectioned, short, want in cases:
            names = ["rle8m_decompress"] if sectioned else ["rle8_low_entropy_decompress"] + (["rle8_low_entropy_short_decompress"] if short else [])
            for fname in names:
                got, buf = ref_decode(reference.lib, fname, stream)
                if got != len(want) or buf[: len(want)] != want:
                    bad.append((level, name, fname, got))
    return bad


def job_all_256(reference, stream, n_want, data):
    res = {}
    got, buf = ref_decode(reference.lib, "rle8_low_entropy_decompress", stream, in_pad=n_want + PAD)
    res["grammar"] = (got, buf[:n_want])
    for variant in range(4):
        s = reference.low_entropy_compress(variant, data)
        got, buf = ref_decode(reference.lib, "rle8_low_entropy_short_decompress" if variant & 1 else "rle8_low_entropy_decompress", s, in_pad=len(data) + PAD)
        res[variant] = (s, buf[: len(data)])
    s = reference.rle8m_compress(2, data)
    got, buf = ref_decode(reference.lib, "rle8m_decompress", s, in_pad=len(data) + PAD)
    res["rle8m"] = (s, buf[: len(data)])
    return res


def job_decode(reference, calls):
    return [ref_decode(reference.lib, fname, stream, in_size) for fname, stream, in_size in calls]


JOBS = {"agree": job_agree, "all_256": job_all_256, "decode": job_decode}


def in_child(tmp_path, job, *args):
    """JOBS[job](Reference(), *args) in a fresh interpreter; its result, or a failed assertion when the child did not live to tell"""
    src, dst = tmp_path / "job.pkl", tmp_path / "result.pkl"
    with open(src, "wb") as f:
        pickle.dump((job, args), f)
    run = subprocess.run([sys.executable, os.path.abspath(__file__), str(src), str(dst)], capture_output=True, text=True)
    assert run.returncode == 0 and dst.exists(), f"the reference ended its process (status {run.returncode}): {run.stderr[-2000:]}"
    with open(dst, "rb") as f:
        return pickle.load(f)


def test_reference_agrees_below_256_flags(reference, tmp_path):
    """the plain decoder and rle8m_decompress on every well-formed fixture with fewer than 256 flags (inSize == compressedSize), the Short decoder
    on those whose counts are all <= 31"""
    cases = []
    for name, stream, sectioned in all_well_formed():
        out, forms = parsed(name, stream, sectioned)
        if forms["flags.256"]:
            continue
        short = not sectioned and all(int(k[4:]) <= 31 for k in forms if k.startswith("cnt."))
        cases.append((name, stream, sectioned, short, out))
    assert sum(c[3] for c in cases) >= 5 and len(cases) > 80
    assert in_child(tmp_path, "agree", cases) == []


def test_reference_departure_all_256_flags(reference, oracle, tmp_path):
    """its flag counter is a uint8_t: 256 flags read as none and the stream is copied raw.  An encoder gets there: the reference does not give
    its own streams of ALL_256_INPUT back, the oracle does."""
    data = G.ALL_256_INPUT
    assert len(data) == 2304
    stream = G.le_fixtures()["form.flags.256"]
    want = G.model(stream, False)
    res = in_child(tmp_path, "all_256", stream, len(want), data)
    body_at = 8 + 33 + 255
    assert res["grammar"][1] != want and res["grammar"][1] == (stream[body_at:] + b"\x55" * len(want))[: len(want)], "the reference no longer copies a 256-flag stream raw"
    for key in (0, 1, 2, 3, "rle8m"):
        s, back = res[key]
        sectioned = key == "rle8m"
        if key == 0:
            assert len(s) == 1834
        forms = G.parse(s, sectioned)[1]
        if key in (0, 1, "rle8m"):
            assert forms["flags.256"] == 1, key
            assert back != data, f"{key}: the reference round-trips its 256-flag stream now"
        assert G.model(s, sectioned) == data
        got, buf = oracle_decode(oracle, s, sectioned)
        assert got == len(data) and buf[: len(data)] == data, key


def test_reference_departure_short_decoder_above_31(reference, tmp_path):
    """the Short decoder's vector loops write 32 bytes per token whatever the count says: a count above 31 leaves a hole"""
    h = G.HF
    stream = h.le(G.Body(h).plain(20).tok(G.F2, 100, None).plain(400))
    want = G.model(stream, False)
    (got_s, buf_s), (got_p, buf_p) = in_child(tmp_path, "decode", [("rle8_low_entropy_short_decompress", stream, None), ("rle8_low_entropy_decompress", stream, None)])
    assert got_p == len(want) and buf_p[: len(want)] == want
    assert buf_s[: len(want)] != want and buf_s[:53] == want[:53] and buf_s[53:121] == b"\xEE" * 68, "the reference's Short decoder follows counts above 31 now"


def test_reference_departure_rle8m_last_section_ends_at_in_size(reference, oracle, tmp_path):
    """rle8m_decompress ends the last section at pIn + inSize, not at the header's compressed size: bytes behind the stream are decoded too"""
    h = G.HF
    sec = G.Body(h).plain(30).tok(G.F2, 5, None).plain(10)
    stream = h.rle8m([sec, sec])
    want = G.model(stream, True)
    extra = bytes(h.plain[:8])
    ((got, buf),) = in_child(tmp_path, "decode", [("rle8m_decompress", stream + extra, len(stream) + 8)])
    assert got == len(want) and buf[: len(want)] == want
    assert buf[len(want) : len(want) + 8] == extra, "the reference's rle8m_decompress stops at the compressed size now"
    got, buf = oracle_decode(oracle, stream + extra, True)
    assert got == len(want) and buf[: len(want)] == want and buf[len(want) :] == b"\xEE" * PAD


# ------------------------------------------------------------------------------------------------------------------
# the oracle's decoders under the address and undefined-behaviour sanitizers (a stand-alone program on the CPU)


def test_oracle_decoders_under_the_sanitizers(tmp_path):
    """tests/low_entropy_sanitize_main.c + oracle/hsrle_oracle.c built with -fsanitize=address,undefined: every malformed stream is refused and
    every small well-formed one decoded with streams and outputs in heap blocks of their exact size, and the sanitizers stay silent"""
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    if subprocess.run([cc] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot build with the sanitizers")
    here = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "le_sanitize")
    build = subprocess.run([cc, "-O1", "-g", "-std=gnu99"] + flags + [os.path.join(here, "low_entropy_sanitize_main.c"),
                            os.path.join(here, "..", "oracle", "hsrle_oracle.c"), os.path.join(here, "..", "oracle", "hsrle_synth.c"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    records = []
    for sectioned, fx in ((False, G.le_malformed()), (True, G.rle8m_malformed())):
        records += [(sectioned, stream, 0) for stream, _ in fx.values()]
    for name, stream, sectioned in all_well_formed():
        if len(stream) < 20000:
            records.append((sectioned, stream, struct.unpack_from("<I", stream, 4)[0]))
    for cut in (0, 1, 7, 8, 11, 12, 40, 41, 48):                           # ... and streams shorter than their own header
        records += [(False, G.le_fixtures()["size.1"][:cut], 0), (True, G.rle8m_fixtures()["edges.hf.2.mid"][:cut], 0)]
    path = tmp_path / "streams.bin"
    with open(path, "wb") as f:
        for sectioned, stream, want in records:
            f.write(struct.pack("<BII", sectioned, len(stream), want) + stream)
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert f"{len(records)} records" in run.stdout


if __name__ == "__main__":                                               # the child of in_child
    from hsrle_testlib import Reference

    with open(sys.argv[1], "rb") as f:
        job, args = pickle.load(f)
    result = JOBS[job](Reference(), *args)
    with open(sys.argv[2], "wb") as f:
        pickle.dump(result, f)
