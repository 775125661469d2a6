#!/usr/bin/env python3
"""Mint tests/golden/mmtf/vectors.json from the COMPILED reference (oracle/_ref/libhsrle_ref.so, built by oracle/Makefile where the reference's
sources are present): small inputs with the bytes the reference's mmtf128 / mmtf256 / bitmmtf8 / bitmmtf16 encode and decode functions give
for them.  Data only; tests/test_mmtf_model.py holds the Python model against it on machines without the reference."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from mmtf_testlib import GOLDEN_DIR, NAMES, TRANSFORMS, MmtfReference, random_bytes  # noqa: E402

INPUTS = (("empty", 0, 1), ("one", 1, 256), ("n17_a5", 17, 5), ("n45_a5", 45, 5), ("n130_a256", 130, 256), ("n200_a3", 200, 3))


def main():
    if not MmtfReference.available():
        print("oracle/_ref/libhsrle_ref.so is missing: build it with `make -C oracle` where the reference's sources are present")
        return 1
    ref = MmtfReference()
    vectors = []
    for name, n, alphabet in INPUTS:
        data = random_bytes(n, alphabet, 11)
        v = {"name": name, "input": data.hex()}
        for t in TRANSFORMS:
            for decode in (0, 1):
                rc, out = ref.run(t, decode, data)
                assert rc == n, (name, t, decode, rc)
                v[NAMES[t] + ("_decode" if decode else "_encode")] = out.hex()
        vectors.append(v)
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    with open(os.path.join(GOLDEN_DIR, "vectors.json"), "w") as f:
        json.dump({"source": "compiled reference: mmtf.c, bit_mmtf.c", "vectors": vectors}, f, indent=1)
        f.write("\n")
    print(f"wrote {len(vectors)} vectors")
    return 0


if __name__ == "__main__":
    sys.exit(main())
