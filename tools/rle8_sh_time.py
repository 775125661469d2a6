#!/usr/bin/env python3
"""Device time of the rle8_sh codec (hsrle_rle8_sh_compress_dev_async / _decompress_dev_async), both directions, on device-resident data:
run-distributed and video-shaped hsrle_synth_dev bytes, and random bytes (the stream is the input plus 18 bytes: one raw COPY).

Per row: the median of --reps timed enqueues (HIP events, 2 warm-ups), next to the compiled reference's rate on ONE core of the same machine on
the first --ref-mib MiB of the same bytes (oracle/_ref/libhsrle_ref.so, when present).
Checks: the device status words, decompress(compress(x)) == x on the device for the whole buffer, and -- with the reference -- that the library's
stream of the first --ref-mib MiB equals the reference's byte for byte.  `guess failed`: stretches whose proof of the decoder's guess failed (0 is expected
of every encoder-made stream; then the serial fallback did not run).
Per-kernel times: run the same command with --once under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/rle8_sh_time.py --once):
every kernel then runs exactly once per input and direction, after one warm-up.

  python tools/rle8_sh_time.py [--gib 1] [--reps 5] [--ref-mib 64] [--out profiles/r12_rle8_sh.md]
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
import torch  # noqa: E402
import hsrle  # noqa: E402
import rle8_sh_testlib as T  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, reps, warm):
    t = [timed(fn) for _ in range(reps + warm)][warm:]
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-mib", type=int, default=64)
    ap.add_argument("--inputs", default="runs,video,random")
    ap.add_argument("--once", action="store_true", help="one warm-up and one timed enqueue per row (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = min(int(args.gib * (1 << 30)), 1 << 30)
    reps, warm = (1, 1) if args.once else (max(args.reps, 3), 2)
    m = min(n, args.ref_mib << 20)
    ref = T.Rle8ShReference() if T.Rle8ShReference.available() else None
    hsrle.rle8_sh_tuning(0, 0, 0)
    GiB = float(1 << 30)
    rows, ok = [], True
    cap = hsrle.rle8_sh_capacity(n)
    enc = torch.empty(cap, dtype=torch.uint8, device="cuda")
    dec = torch.empty(n, dtype=torch.uint8, device="cuda")
    words = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    wsc = torch.full((hsrle.rle8_sh_workspace_size(0, n),), 0xC3, dtype=torch.uint8, device="cuda")
    wsd = torch.full((hsrle.rle8_sh_workspace_size(1, n),), 0xC3, dtype=torch.uint8, device="cuda")
    for kname in args.inputs.split(","):
        if kname == "random":
            src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        else:
            src = hsrle.synth(hsrle.SYNTH_VIDEO if kname == "video" else hsrle.SYNTH_RUNS, 1, 2, n, device="cuda")
        ref_rate, ref_ok = {0: None, 1: None}, None
        if ref is not None:
            host = src[:m].cpu().numpy().tobytes()
            t0 = time.perf_counter()
            theirs = ref.compress(host)
            ref_rate[0] = m / GiB / (time.perf_counter() - t0)
            t0 = time.perf_counter()
            back = ref.decompress(theirs, m)
            ref_rate[1] = m / GiB / (time.perf_counter() - t0)
            hsrle.rle8_sh_compress_dev(src[:m], enc, words[0:1], words[1:2], wsc)
            torch.cuda.synchronize()
            mine = enc[: int(words[0].item())].cpu().numpy().tobytes()
            ref_ok = back == (m, host) and mine == theirs
            ok = ok and ref_ok
        hsrle.rle8_sh_compress_dev(src, enc, words[0:1], words[1:2], wsc)
        torch.cuda.synchronize()
        size, status = int(words[0].item()), int(words[1].item())
        if status != hsrle.RLE8_SH_DONE:
            sys.exit(f"{kname}: compress status {status}")
        stream = enc[:size]
        hsrle.rle8_sh_decompress_dev(stream, dec, words[2:3], wsd)
        torch.cuda.synchronize()
        round_trip = int(words[2].item()) == hsrle.RLE8_SH_DONE and bool(torch.equal(dec, src))
        fallback, failed = hsrle.rle8_sh_decode_words(wsd)
        ok = ok and round_trip
        for decode in (0, 1):
            if decode:
                med, lo, hi = median_ms(lambda: hsrle.rle8_sh_decompress_dev(stream, dec, words[2:3], wsd), reps, warm)
            else:
                med, lo, hi = median_ms(lambda: hsrle.rle8_sh_compress_dev(src, enc, words[0:1], words[1:2], wsc), reps, warm)
            row = {"direction": "decompress" if decode else "compress", "input": kname, "bytes": n, "stream_bytes": size, "ms": round(med, 3),
                   "spread_ms": [round(lo, 3), round(hi, 3)], "gpu_GiBps": round(n / GiB / (med / 1e3), 3),
                   "ref_GiBps": None if ref_rate[decode] is None else round(ref_rate[decode], 3), "reference_agrees": ref_ok, "round_trip": round_trip,
                   "decode_fallback_ran": fallback, "failed_proofs": failed}
            rows.append(row)
            print(json.dumps(row), flush=True)
        del src
        torch.cuda.empty_cache()
    lines = [f"# rle8_sh on the GPU ({n / GiB:g} GiB device resident, median of {reps} timed enqueues after {warm} warm-ups, HIP events)", "",
             f"build id: {hsrle.build_id()}  device: {torch.cuda.get_device_name(0)}", "",
             f"reference: compiled reference on one core, first {m >> 20} MiB of the same bytes; `agrees`: the library's stream of them equals the reference's.", "",
             "| direction | input | stream / input | GPU ms | GPU GiB/s | reference 1 core GiB/s | GPU / reference | reference agrees | round trip | guess failed |",
             "|---|---|---:|---:|---:|---:|---:|---|---|---:|"]
    for r in rows:
        rr = r["ref_GiBps"]
        lines.append(f"| {r['direction']} | {r['input']} | {r['stream_bytes'] / r['bytes']:.4f} | {r['ms']:.3f} | {r['gpu_GiBps']:.3f} | "
                     f"{('%.3f' % rr) if rr else 'n/a'} | {('%.2f' % (r['gpu_GiBps'] / rr)) if rr else 'n/a'} | "
                     f"{'n/a' if r['reference_agrees'] is None else ('yes' if r['reference_agrees'] else 'NO')} | {'yes' if r['round_trip'] else 'NO'} | {r['failed_proofs']} |")
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
