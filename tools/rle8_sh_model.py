#!/usr/bin/env python3
"""The rle8_sh encoder's decisions as a loop over MAXIMAL RUNS of equal bytes (tests/rle8_sh_testlib.py: model_compress), held against the
reference's byte loop restated (model_compress_bytewise) and, where oracle/_ref/libhsrle_ref.so is built, against the compiled reference.  This is
what csrc/hsrle_rle8sh.hip.h: k_she_decide runs: one step per run, the same counters; its shortcut over whole words of short runs is restated
too (model_compress_words) and held against the same streams.

  pend       length of an R-run that has not been emitted: part of the open block, or a FILL to come
  change     length of the last run if it was not of R: 10 and more make its symbol the new R when the next run begins
  rInBlock   bytes of R in the open block, for the 7 : 2 rule (7 * R bytes > 2 * other bytes: the block is coded symbol by symbol)
It also reports the largest items / size and stream - size it meets: the bounds of the workspace plan and of hsrle_rle8_sh_capacity.

  python tools/rle8_sh_model.py [--trials 2000]
"""
import argparse
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import rle8_sh_testlib as T  # noqa: E402


def capacity(n):
    return n + n // 221 + 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=2000)
    args = ap.parse_args()
    ref = T.Rle8ShReference() if T.Rle8ShReference.available() else None
    rng = random.Random(1)
    inputs = list(T.input_set().values())
    for t in range(args.trials):
        inputs.append(T.geometric_runs(rng.randrange(1, 3000), rng.choice((1, 2, 3, 4, 8, 256)), t, mean=rng.choice((2, 6, 12, 20))))
    inputs.append(T.short_coded_stretches(3000))
    inputs.append(T.raw_blocks_between_changes(6000))
    inputs.append(T.marginal_encoded_spans(2000))
    worst_items, worst_growth, shortcuts = 0.0, -10**9, 0
    for d in inputs:
        by_run, items = T.model_compress(d)
        by_byte, items2 = T.model_compress_bytewise(d)
        assert by_run == by_byte and items == items2, "the run-level loop differs from the byte loop"
        by_word, items3, cut = T.model_compress_words(d)
        assert by_word == by_run and items3 == items, "the decision kernel's shortcut over whole words changes the stream"
        shortcuts += cut
        if ref is not None:
            assert by_run == ref.compress(d), "the model differs from the compiled reference"
        assert T.model_decompress(by_run) == d
        assert len(by_run) <= capacity(len(d)), (len(d), len(by_run))
        spans = sum(1 for k, _, _ in items if k != "enc") + 1           # (the kernel keeps an encoded copy as ONE item)
        if len(d) >= 50:
            worst_items = max(worst_items, spans / len(d))
        worst_growth = max(worst_growth, len(by_run) - capacity(len(d)))
    print(f"{len(inputs)} inputs: run-level == byte loop" + (" == compiled reference" if ref else " (compiled reference not built)"))
    print(f"the shortcut over whole words of short runs was taken {shortcuts} times and changed nothing")
    print(f"largest items / size (size >= 50): {worst_items:.4f} (plan: 0.2); stream size - capacity at the closest: {worst_growth}")


if __name__ == "__main__":
    main()
