"""Mints tests/golden/rle8_mmtf/vectors.json from the compiled reference (oracle/_ref/libhsrle_ref.so, built by oracle/Makefile): small inputs and the
reference's rle8_mmtf128_compress stream for each, as hex.  The streams are SNAPSHOTS: the reference ORs an undefined start value into the width of
the first COPY packet, so another build of it may give another first width; every snapshot is a legal stream all the same.
    python tests/golden/make_rle8_mmtf_golden.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import rle8_mmtf_testlib as T  # noqa: E402
from mmtf_testlib import every_symbol_per_column, video_shaped  # noqa: E402


def inputs():
    rng = random.Random(11)
    out = [("zeros_%d" % n, bytes(n)) for n in (1, 15, 16, 17, 48)]
    out += [("fives_16", b"\x05" * 16), ("random_33", rng.randbytes(33)), ("random_600", rng.randbytes(600))]
    for a in (1, 2, 3, 5, 17, 256):
        out.append((f"alphabet{a}_700", T.random_alphabet(700, a, 2)))
    out.append(("every_symbol", every_symbol_per_column(16 * 270 + 3, 16)))
    out.append(("video_1500", video_shaped(1500)))
    for top in (3, 7, 15, 200):
        for c in (1, 3, 4, 5, 6, 7, 13):
            spec = [("copy", c, top), ("rle", 2, 1), ("copy", c, top), ("rle", 1, 0), ("rle", 1, 2)]
            out.append((f"packets_top{top}_rows{c}", T.data_from_rank_rows(T.rows_from_spec(spec, seed=c), b"\x00\x03\x01")))
    out.append(("headers_32_128", T.data_from_rank_rows(T.rows_from_spec([("copy", 32, 3), ("rle", 128, 4), ("copy", 31, 9), ("rle", 127, 0)]))))
    return out


def main():
    ref = T.Rle8MmtfReference()
    vectors = []
    for name, data in inputs():
        stream = ref.compress(data)
        assert ref.decompress(stream, len(data)) == (len(data), data), name
        vectors.append({"name": name, "input": data.hex(), "stream": stream.hex()})
    path = T.GOLDEN
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"source": "rle8_mmtf128_compress of the compiled reference (oracle/Makefile's recipe)", "vectors": vectors}, f, indent=0)
        f.write("\n")
    print(f"{len(vectors)} vectors -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
