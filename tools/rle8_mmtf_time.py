#!/usr/bin/env python3
"""Device time of the rle8_mmtf128 codec (hsrle_rle8_mmtf128_compress_dev_async / _decompress_dev_async), both directions, on device-resident data:
video-shaped and run-distributed hsrle_synth_dev bytes, and a stream of MANY TINY PACKETS (one literal row, one uniform row, in turn) that shows
what the decode's one-wave header walk costs when nothing else is left to do.

Per row: the median of --reps timed enqueues (HIP events, 2 warm-ups), next to
  * the bare mmtf128 transform of the same bytes in the same direction (hsrle_mmtf_dev_async) and the ratio -- the codec is expected to cost little over it,
  * the compiled reference's rate on ONE core of the same machine on the first --ref-mib MiB of the same bytes (oracle/_ref/libhsrle_ref.so, when present).
Checks: the device status words, decompress(compress(x)) == x on the device for the whole buffer, and the reference's decoder restores the first
--ref-mib MiB from the library's stream of them.
Per-kernel times: run the same command with --once under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/rle8_mmtf_time.py --once):
every kernel then runs exactly once per input and direction, after one warm-up.

  python tools/rle8_mmtf_time.py [--gib 1] [--reps 7] [--ref-mib 64] [--out profiles/r09_rle8_mmtf.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hypersonic-rle-kit_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hsrle  # noqa: E402
import rle8_mmtf_testlib as T  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, reps, warm=2):
    t = [timed(fn) for _ in range(reps + warm)][warm:]
    return statistics.median(t), min(t), max(t)


def tiny_packets(n):
    """Row 2k: a literal row whose ranks stay below 4; row 2k + 1: a uniform row.  As INPUT bytes: every column alternates between two symbols
    in a pattern that makes the ranks (0 1 0 1 ...) on even rows and all 1 on odd rows."""
    rows = n // 16
    ranks = torch.ones((rows, 16), dtype=torch.uint8, device="cuda")
    ranks[0::2, 0::2] = 0
    ranks = ranks.reshape(-1)
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    ws = torch.empty(hsrle.mmtf_workspace_size(hsrle.MMTF128, rows * 16), dtype=torch.uint8, device="cuda")
    hsrle.mmtf_dev(hsrle.MMTF128, 1, ranks, src, ws)      # the inverse transform of the ranks wanted
    src[rows * 16 :] = 0
    torch.cuda.synchronize()
    return src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ref-mib", type=int, default=64)
    ap.add_argument("--inputs", default="video,runs,tiny_packets")
    ap.add_argument("--once", action="store_true", help="one warm-up and one timed enqueue per row (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = min(int(args.gib * (1 << 30)), 1 << 30)
    reps, warm = (1, 1) if args.once else (max(args.reps, 3), 2)
    m = min(n, args.ref_mib << 20) & ~63
    ref = T.Rle8MmtfReference() if T.Rle8MmtfReference.available() else None
    hsrle.mmtf_tuning(0)
    hsrle.rle8_mmtf_tuning(0)
    GiB = float(1 << 30)
    rows, ok = [], True
    enc = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    dec = torch.empty(n, dtype=torch.uint8, device="cuda")
    ranks = torch.empty(n, dtype=torch.uint8, device="cuda")
    words = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    wsc = torch.full((hsrle.rle8_mmtf128_workspace_size(0, n),), 0xC3, dtype=torch.uint8, device="cuda")
    wsd = torch.full((hsrle.rle8_mmtf128_workspace_size(1, n),), 0xC3, dtype=torch.uint8, device="cuda")
    wsm = wsd[: hsrle.mmtf_workspace_size(hsrle.MMTF128, n)]
    for kname in args.inputs.split(","):
        src = tiny_packets(n) if kname == "tiny_packets" else hsrle.synth(hsrle.SYNTH_VIDEO if kname == "video" else hsrle.SYNTH_RUNS, 1, 2, n, device="cuda")
        hsrle.rle8_mmtf128_compress_dev(src, enc, words[0:1], words[1:2], wsc)
        torch.cuda.synchronize()
        size, status = int(words[0].item()), int(words[1].item())
        if status != hsrle.RLE8_MMTF_DONE:
            sys.exit(f"{kname}: compress status {status}")
        stream = enc[:size]
        hsrle.rle8_mmtf128_decompress_dev(stream, dec, words[2:3], wsd)
        torch.cuda.synchronize()
        round_trip = int(words[2].item()) == hsrle.RLE8_MMTF_DONE and bool(torch.equal(dec, src))
        ok = ok and round_trip
        ref_rate, ref_ok = {0: None, 1: None}, None
        if ref is not None:
            host = src[:m].cpu().numpy().tobytes()
            t0 = time.perf_counter()
            theirs = ref.compress(host)
            ref_rate[0] = m / GiB / (time.perf_counter() - t0)
            t0 = time.perf_counter()
            back = ref.decompress(theirs, m)
            ref_rate[1] = m / GiB / (time.perf_counter() - t0)
            hsrle.rle8_mmtf128_compress_dev(src[:m], enc, words[0:1], words[1:2], wsc)
            torch.cuda.synchronize()
            mine = enc[: int(words[0].item())].cpu().numpy().tobytes()
            ref_ok = back == (m, host) and ref.decompress(mine, m) == (m, host) and mine[T.first_copy_end(mine) :] == theirs[T.first_copy_end(theirs) :]
            ok = ok and ref_ok
            hsrle.rle8_mmtf128_compress_dev(src, enc, words[0:1], words[1:2], wsc)
            torch.cuda.synchronize()
        for decode in (0, 1):
            if decode:
                med, lo, hi = median_ms(lambda: hsrle.rle8_mmtf128_decompress_dev(stream, dec, words[2:3], wsd), reps, warm)
                hsrle.mmtf_dev(hsrle.MMTF128, 0, src, ranks, wsm)
                bare, _, _ = median_ms(lambda: hsrle.mmtf_dev(hsrle.MMTF128, 1, ranks, dec, wsm), reps, warm)
            else:
                med, lo, hi = median_ms(lambda: hsrle.rle8_mmtf128_compress_dev(src, enc, words[0:1], words[1:2], wsc), reps, warm)
                bare, _, _ = median_ms(lambda: hsrle.mmtf_dev(hsrle.MMTF128, 0, src, dec, wsm), reps, warm)
            row = {"direction": "decompress" if decode else "compress", "input": kname, "bytes": n, "stream_bytes": size, "ms": round(med, 3),
                   "spread_ms": [round(lo, 3), round(hi, 3)], "gpu_GiBps": round(n / GiB / (med / 1e3), 2), "bare_mmtf128_ms": round(bare, 3),
                   "over_bare": round(med / bare, 2), "ref_GiBps": None if ref_rate[decode] is None else round(ref_rate[decode], 3),
                   "reference_agrees": ref_ok, "round_trip": round_trip}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del src
        torch.cuda.empty_cache()
    lines = [f"# rle8_mmtf128 on the GPU ({n / GiB:g} GiB device resident, median of {reps} timed enqueues after {warm} warm-ups, HIP events)", "",
             f"build id: {hsrle.build_id()}  device: {torch.cuda.get_device_name(0)}", "",
             f"bare mmtf128: hsrle_mmtf_dev_async alone on the same bytes, same direction; reference: compiled reference on one core, first {m >> 20} MiB.", "",
             "| direction | input | stream / input | GPU ms | GPU GiB/s | bare mmtf128 ms | codec / bare | reference 1 core GiB/s | reference agrees | round trip |",
             "|---|---|---:|---:|---:|---:|---:|---:|---|---|"]
    for r in rows:
        rr = r["ref_GiBps"]
        lines.append(f"| {r['direction']} | {r['input']} | {r['stream_bytes'] / r['bytes']:.4f} | {r['ms']:.3f} | {r['gpu_GiBps']:.2f} | {r['bare_mmtf128_ms']:.3f} | {r['over_bare']:.2f} | "
                     f"{('%.3f' % rr) if rr else 'n/a'} | {'n/a' if r['reference_agrees'] is None else ('yes' if r['reference_agrees'] else 'NO')} | {'yes' if r['round_trip'] else 'NO'} |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if not ok:
        sys.exit("outputs differ")


if __name__ == "__main__":
    main()
