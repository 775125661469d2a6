#!/usr/bin/env python3
"""Device time of the monolithic ENCODE of the codecs that moved to the windowed chunk mode (csrc/hsrle_encodeSpw.hip.h): the old flow (cut finder,
host read-back, ring encoders in MONO mode, staging slots, host list rounds) against the new one, synchronous (hsrle_compress_mono_dev) and
enqueue-only (hsrle_compress_mono_dev_enqueue), on 1 GiB run-distributed and video-shaped synthetic inputs.

Needs an experiments build (-DHSRLE_EXPERIMENTS; HSRLE_LIB=<its path>): there HSRLE_PP=2 forces the old flow, in the same process, so old and new
alternate call by call.  Every row is checked byte for byte: the new streams (both entry points) against the old flow's.
HIP events around each call, 2 warm-ups, the median of --reps (>= 10).

  HSRLE_LIB=variants/libhsrle_exp.so python tools/mono_encode_time.py [--keys k1,k2] [--gib 1] [--reps 11] [--out FILE.md]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hypersonic-rle-kit_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402
import hsrle  # noqa: E402
from hsrle_testlib import CODEC_BY_KEY  # noqa: E402

KEYS = ["rle16_sym_packed", "rle32_byte_packed", "rle64_sym", "rle24_byte_short", "rle48_1symlut_sym_short", "rle8_multi_short"]


def old_flow(on):
    if on:
        os.environ["HSRLE_PP"] = "2"
    else:
        os.environ.pop("HSRLE_PP", None)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", default=",".join(KEYS))
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not hsrle.experiments_enabled():
        sys.exit("needs an experiments build (-DHSRLE_EXPERIMENTS) through HSRLE_LIB: the old flow is reached with HSRLE_PP=2 there")
    n = int(args.gib * (1 << 30))
    reps = max(args.reps, 10)
    rows = []
    for key in args.keys.split(","):
        codec = CODEC_BY_KEY[key]
        for kind, kname in ((hsrle.SYNTH_RUNS, "runs"), (hsrle.SYNTH_VIDEO, "video")):
            src = hsrle.synth(kind, codec.S, 2, n, device="cuda")
            cap = hsrle.compress_bounds(n) + 64
            old_flow(True)
            ws_old = torch.empty(hsrle.mono_compress_workspace_size(key, n), dtype=torch.uint8, device="cuda")
            old_flow(False)
            ws_new = torch.empty(hsrle.mono_compress_workspace_size(key, n), dtype=torch.uint8, device="cuda")
            d_old, d_new, d_enq = (torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(3))
            status, size = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
            out = {}

            def run_old():
                old_flow(True)
                out["old"] = hsrle.mono_compress_dev(key, src, dst=d_old, workspace=ws_old).numel()
                old_flow(False)

            def run_new():
                out["new"] = hsrle.mono_compress_dev(key, src, dst=d_new, workspace=ws_new).numel()

            def run_enq():
                hsrle.mono_compress_dev_enqueue(key, src, d_enq, ws_new, status, size)

            t = {"old": [], "new": [], "enqueue": []}
            for r in range(reps + 2):
                for name, fn in (("old", run_old), ("new", run_new), ("enqueue", run_enq)):
                    ms = timed(fn)
                    if r >= 2:
                        t[name].append(ms)
            c = out["old"]
            same = (out["new"] == c and int(size.item()) == c and int(status.item()) == hsrle.MONO_DONE and torch.equal(d_new[:c], d_old[:c])
                    and torch.equal(d_enq[:c], d_old[:c]))
            med = {k: statistics.median(v) for k, v in t.items()}
            row = {"codec": key, "input": kname, "bytes": n, "stream": c, "old_ms": round(med["old"], 3), "new_ms": round(med["new"], 3),
                   "enqueue_ms": round(med["enqueue"], 3), "speedup": round(med["old"] / med["new"], 2), "identical": bool(same),
                   "spread_new_ms": [round(min(t["new"]), 3), round(max(t["new"]), 3)], "spread_old_ms": [round(min(t["old"]), 3), round(max(t["old"]), 3)]}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del src, ws_old, ws_new, d_old, d_new, d_enq
            torch.cuda.empty_cache()
    lines = [f"# Monolithic encode, old flow against the windowed chunk mode ({args.gib:g} GiB, median of {reps}, HIP events)", "",
             f"build id: {hsrle.build_id()} (experiments build; HSRLE_PP=2 = old flow)  device: {torch.cuda.get_device_name(0)}", "",
             "| codec | input | stream bytes | old ms | new ms (sync) | new ms (enqueue) | old / new | bytes identical |",
             "|---|---|---:|---:|---:|---:|---:|---|"]
    for r in rows:
        lines.append(f"| {r['codec']} | {r['input']} | {r['stream']} | {r['old_ms']:.3f} | {r['new_ms']:.3f} | {r['enqueue_ms']:.3f} | {r['speedup']:.2f} | {'yes' if r['identical'] else 'NO'} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if not all(r["identical"] for r in rows):
        sys.exit("streams differ")


if __name__ == "__main__":
    main()
