#!/usr/bin/env python3
"""Seekable monolithic streams: what the persistent entry-point index (hsrle_mono_index_build_dev) buys on the 1 GiB rle8_packed stream of
bench.py's extras.mono_1GiB, against the monolithic decode that rebuilds its index on every call (hsrle_decompress_mono_dev).

    python tools/mono_index_time.py [--size-mib N] [--spacing S] [--reps R] [--seed X]

The stream is written on the device by hsrle_compress_mono_dev (byte-identical with the reference encoder's, tests/test_gpu_mono_async.py)
from the run-distributed synthetic input.  Every result is checked against the input.  Prints ONE JSON line (milliseconds, medians of --reps):
  build_ms           index build (synchronous, host wall clock)
  full_range_ms      the whole stream through the prebuilt index (device events)
  range_ms           {"4KiB", "1MiB", "64MiB"}: ranges at seeded random offsets (device events)
  mono_dev_ms        hsrle_decompress_mono_dev on the same stream (synchronous, host wall clock): the baseline
  mono_dev_async_ms  hsrle_decompress_mono_dev_async (index passes + decode, device events)
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hypersonic-rle-kit_amd", "python"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-mib", type=int, default=1024)
    ap.add_argument("--spacing", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    import torch
    import hsrle

    key = "rle8_packed_multi"
    size = args.size_mib << 20
    src = hsrle.synth(hsrle.SYNTH_RUNS, 1, 8, size, device="cuda:0")
    enc = hsrle.mono_compress_dev(key, src)
    csize = enc.numel()
    stream = torch.zeros(csize + 64, dtype=torch.uint8, device="cuda")       # 128-byte aligned, 64 bytes of slack
    stream[:csize] = enc
    del enc
    torch.cuda.synchronize()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    # index build
    index, info = hsrle.mono_index_build(key, stream, spacing=args.spacing)
    ws = torch.empty(hsrle.lib().hsrle_mono_index_workspace_size(hsrle.codec_id(key), size, csize, args.spacing) + 256, dtype=torch.uint8, device="cuda")
    build = [wall(lambda: hsrle.mono_index_build(key, stream, spacing=args.spacing, index=index, workspace=ws))[0] for _ in range(args.reps)]

    out = torch.empty(size, dtype=torch.uint8, device="cuda")
    status = torch.zeros(4, dtype=torch.uint8, device="cuda")

    def check(off, n, dst):
        w = int.from_bytes(status.cpu().numpy().tobytes(), "little")
        assert w == hsrle.MONO_DONE, f"range [{off}, +{n}): status {w}"
        assert torch.equal(dst[:n], src[off : off + n]), f"range [{off}, +{n}) differs"

    # full range through the index
    full = []
    for _ in range(args.reps + 1):
        out.fill_(0)
        full.append(events(lambda: hsrle.mono_decompress_range_dev_async(stream, index, info, 0, size, out, status)))
        check(0, size, out)
    full = full[1:]

    rng = random.Random(args.seed)
    ranges = {}
    for name, n in (("4KiB", 4096), ("1MiB", 1 << 20), ("64MiB", 64 << 20)):
        ts = []
        for _ in range(args.reps + 1):
            off = rng.randrange(size - n + 1)
            dst = out[:n]
            ts.append(events(lambda: hsrle.mono_decompress_range_dev_async(stream, index, info, off, n, dst, status)))
            check(off, n, dst)
        ranges[name] = round(statistics.median(ts[1:]), 4)

    # baseline: the monolithic decode that walks, proves and records on every call
    mws = torch.empty(hsrle.mono_decompress_workspace_size(key, size, csize), dtype=torch.uint8, device="cuda")
    mono = []
    for _ in range(args.reps + 1):
        dt, res = wall(lambda: hsrle.mono_decompress_dev(key, stream, dst=out, workspace=mws))
        mono.append(dt)
    assert torch.equal(out, src)
    head = stream[:16].cpu().numpy().tobytes()
    st32 = torch.zeros(1, dtype=torch.int32, device="cuda")
    mono_async = [events(lambda: hsrle.mono_decompress_dev_async(key, stream, head, out, mws, st32)) for _ in range(args.reps + 1)][1:]
    assert int(st32.item()) == hsrle.MONO_DONE and torch.equal(out, src)

    print(json.dumps({
        "tool": "mono_index_time", "codec": key, "size": size, "compressed": csize, "spacing": info.spacing, "index_bytes": int(info.indexBytes),
        "build_ms": round(statistics.median(build), 4), "full_range_ms": round(statistics.median(full), 4), "range_ms": ranges,
        "mono_dev_ms": round(statistics.median(mono[1:]), 4), "mono_dev_async_ms": round(statistics.median(mono_async), 4),
        "full_range_gib_s": round(size / 2**30 / (statistics.median(full) / 1e3), 1), "reps": args.reps,
    }))


if __name__ == "__main__":
    main()
