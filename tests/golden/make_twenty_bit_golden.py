"""Writes tests/golden/twenty_bit_probes.json: what the compiled reference (oracle/_ref/libhsrle_ref.so) decides on the probes of
tests/twenty_bit_probes.py -- per codec the counts whose stored / not-stored decision flips between range 0xFFFFF and 0xFFFFF + 1 (searched
over 2 .. 6 S + 25 bytes, for a listed and for a new symbol), and per probe whether the run was stored and the stream's length and sha256.
Only recorded results.  Run from the repository root after the oracle has been built; the file regenerates byte for byte."""
import functools
import json
import multiprocessing
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import twenty_bit_probes as P  # noqa: E402
from hsrle_testlib import CODEC_BY_KEY, SINGLE_SHORT, Oracle, Reference  # noqa: E402

_ref = _ora = None


def _libs():
    global _ref, _ora
    if _ref is None:
        _ref, _ora = Reference(), Oracle()
    return _ref, _ora


def _encode(codec, data):
    """(stream, run packets) of the reference; the stream decodes back with the reference's own decoder."""
    ref, ora = _libs()
    raw = data.tobytes()
    stream = ref.compress(codec, raw)
    assert stream is not None and ref.decompress(codec, stream, len(raw)) == raw, codec.key
    return stream, ora.run_packets(codec, stream, len(raw))


@functools.lru_cache(maxsize=None)
def _separator_runs(key, variant, sep):
    """Run packets of a probe without its run: 1, or 0 where the codec cannot store the separator (rle8_single_short stores one symbol only)."""
    codec = CODEC_BY_KEY[key]
    runs = _encode(codec, P.build_probe(codec.S, variant, 0, P.GAPS[0], 0, sep))[1]
    assert runs in (0, 1), (key, variant, runs)
    return runs


def _stored(codec, variant, count, gap, sym_index=0, sep=P.SEP_MONO, size=None):
    """(was the probe's run stored, the reference's stream, its run packets)"""
    ref, ora = _libs()
    raw = P.build_probe(codec.S, variant, count, gap, sym_index, sep, size).tobytes()
    stream = ref.compress(codec, raw)
    runs = ora.run_packets(codec, stream, len(raw)) if ref.decompress(codec, stream, len(raw)) == raw else -1
    stored = runs - _separator_runs(codec.key, variant, sep)
    assert stored in (0, 1), (codec.key, variant, count, gap, runs)
    return stored == 1, stream, runs


def mint(key):
    codec = CODEC_BY_KEY[key]
    ref, ora = _libs()
    flips = {v: [c for c in P.count_candidates(codec.S) if _stored(codec, v, c, P.GAPS[0])[0] != _stored(codec, v, c, P.GAPS[1])[0]] for v in P.VARIANTS}
    probes, entries = P.probe_list(codec.S, flips), []
    for p in probes:
        stored, stream, runs = _stored(codec, p.variant, p.count, p.gap, p.sym_index)
        entries.append({"variant": p.variant, "count": p.count, "gap": p.gap, "symbol": p.sym_index, "stored": stored, "run_packets": runs, "length": len(stream),
                        "sha256": P.sha(stream)})
    stream, count_runs = _encode(codec, P.build_count_probe(codec))
    assert count_runs == 2, key
    count_probe = {"count": P.count_probe_bytes(codec), "gap": P.COUNT_GAP, "stored": True, "length": len(stream), "sha256": P.sha(stream)}
    data, used = P.mono_input(codec, probes)
    stream, runs = _encode(codec, data)
    mono = {"probes": used, "size": int(data.size), "run_packets": runs, "length": len(stream), "sha256": P.sha(stream)}
    # every decision as in the probe alone (rle8_single_short stores ONE symbol per stream: here the count probe's, so no 0x33 separator)
    one_symbol = codec.family == SINGLE_SHORT
    assert runs == count_runs + sum(int(entries[i]["stored"]) + (0 if one_symbol and probes[i].variant == "new" else 1) for i in used), key
    blocks = P.container_input(codec, probes).reshape(len(probes), P.BLOCK)
    streams = [_encode(codec, b) for b in blocks]
    decided = [r - _separator_runs(key, p.variant, P.SEP_BLOCK) for (_, r), p in zip(streams, probes)]
    assert decided == [int(e["stored"]) for e in entries], key                             # ... and behind the blocks' shorter separator
    container = {"lengths": [len(s) for s, _ in streams], "sha256": P.sha(b"".join(s for s, _ in streams))}
    return key, {"flips": flips, "probes": entries, "count_probe": count_probe, "mono": mono, "container": container}


def main():
    assert Reference.available(), "build the compiled reference first (make -C oracle)"
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        codecs = dict(pool.map(mint, [c.key for c in P.RULE_CODECS], chunksize=1))
    flipping = sorted(k for k, e in codecs.items() if e["flips"]["listed"] or e["flips"]["new"])
    doc = {"source": "the reference's <codec>_compress on the probes of tests/twenty_bit_probes.py, built by oracle/Makefile",
           "threshold": P.T, "flipping": flipping, "codecs": {c.key: codecs[c.key] for c in P.RULE_CODECS}}
    with open(P.GOLDEN, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    chunk = [k for k in flipping if P.is_chunk_mode_short(CODEC_BY_KEY[k])]
    print(len(flipping), "of", len(codecs), "codecs flip,", len(chunk), "of them chunk-mode Short;", os.path.getsize(P.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
