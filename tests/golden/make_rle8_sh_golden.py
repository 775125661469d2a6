"""Writes tests/golden/rle8_sh/vectors.json: streams of the compiled reference (oracle/_ref/libhsrle_ref.so) with their inputs, so that the GPU tests
have the reference's bytes where the compiled reference is not at hand.  Run from the repository root after the oracle has been built."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import rle8_sh_testlib as T  # noqa: E402


def main():
    ref = T.Rle8ShReference()
    vectors = []
    for name, data in T.input_set().items():
        if len(data) > 1100 and name not in ("alphabet3_3000", "alphabet256_3000", "random_3000"):
            continue
        stream = ref.compress(data)
        n, back = ref.decompress(stream, len(data))
        assert (n, back) == (len(data), data), name
        vectors.append({"name": name, "input": data.hex(), "stream": stream.hex()})
    os.makedirs(os.path.dirname(T.GOLDEN), exist_ok=True)
    with open(T.GOLDEN, "w") as f:
        json.dump({"source": "rle8_sh_compress of the reference (src/rle_sh.c), built by oracle/Makefile", "vectors": vectors}, f, indent=0)
        f.write("\n")
    print(len(vectors), "vectors,", os.path.getsize(T.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
