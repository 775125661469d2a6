#!/usr/bin/env python3
"""Device time of the mmtf128 / mmtf256 / bitmmtf8 / bitmmtf16 transforms (hsrle_mmtf_dev_async), both directions, on device-resident data:
video-shaped and run-distributed hsrle_synth_dev bytes and random bytes (the worst case of a move-to-front list: every rank is as likely as any).

Per row: the median of --reps timed enqueues (HIP events, 2 warm-ups), next to
  * the compiled reference's rate on ONE core of the same machine for the same bytes (oracle/_ref/libhsrle_ref.so, when present), and
  * a device-to-device copy of the same size -- the ceiling of anything that reads and writes every byte once.
Checks: decode(encode(x)) == x on the device for the whole buffer; and the first --ref-mib MiB of every output against the compiled reference run
on the first --ref-mib MiB of the input (every transform here is causal: a prefix of whole rows of the output depends on that prefix of the input only,
so the reference need not chew through the whole GiB on one core to check it, and its rate is taken on that prefix).  The decodes read the encoded form.

  python tools/mmtf_time.py [--gib 1] [--reps 11] [--ref-mib 256] [--out profiles/r08_mmtf.md]
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
import mmtf_testlib as mt  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def median_ms(fn, reps):
    t = []
    for r in range(reps + 2):
        ms = timed(fn)
        if r >= 2:
            t.append(ms)
    return statistics.median(t), min(t), max(t)


def reference_run(ref, transform, decode, host):
    """(seconds on one core, output bytes) of the compiled reference on a host array"""
    n = host.size
    src = np.ascontiguousarray(host)
    dst = np.empty(n + 64, dtype=np.uint8)
    f = getattr(ref.lib, mt.function_name(transform, decode))
    t0 = time.perf_counter()
    rc = f(src.ctypes.data, n, dst.ctypes.data, n)
    dt = time.perf_counter() - t0
    if rc != n:
        sys.exit(f"reference {mt.function_name(transform, decode)} returned {rc}")
    return dt, dst[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--ref-mib", type=int, default=256)
    ap.add_argument("--inputs", default="video,runs,random")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    n = int(args.gib * (1 << 30))
    reps = max(args.reps, 5)
    m = min(n, args.ref_mib << 20) & ~63
    ref = mt.MmtfReference() if mt.MmtfReference.available() else None
    hsrle.mmtf_tuning(0)
    GiB = float(1 << 30)
    rows, ok = [], True
    enc, dec = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    for kname in args.inputs.split(","):
        if kname == "random":
            g = torch.Generator(device="cuda")
            g.manual_seed(5)
            src = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        else:
            src = hsrle.synth(hsrle.SYNTH_VIDEO if kname == "video" else hsrle.SYNTH_RUNS, 1, 2, n, device="cuda")
        copy_ms, _, _ = median_ms(lambda: dec.copy_(src), reps)
        host_src = src[:m].cpu().numpy()
        for transform in mt.TRANSFORMS:
            ws = torch.full((hsrle.mmtf_workspace_size(transform, n),), 0xC3, dtype=torch.uint8, device="cuda")
            hsrle.mmtf_dev(transform, 0, src, enc, ws)
            hsrle.mmtf_dev(transform, 1, enc, dec, ws)
            torch.cuda.synchronize()
            round_trip = bool(torch.equal(dec, src))
            host_enc = enc[:m].cpu().numpy()
            for decode in (0, 1):
                a, b = (enc, dec) if decode else (src, enc)
                med, lo, hi = median_ms(lambda: hsrle.mmtf_dev(transform, decode, a, b, ws), reps)
                row = {"transform": mt.NAMES[transform], "direction": "decode" if decode else "encode", "input": kname, "bytes": n, "ms": round(med, 3),
                       "spread_ms": [round(lo, 3), round(hi, 3)], "gpu_GiBps": round(n / GiB / (med / 1e3), 2), "copy_GiBps": round(n / GiB / (copy_ms / 1e3), 1),
                       "workspace": ws.numel(), "round_trip": round_trip, "ref_GiBps": None, "equals_reference": None}
                if ref is not None:
                    dt, out = reference_run(ref, transform, decode, host_enc if decode else host_src)
                    mine = (dec if decode else enc)[:m].cpu().numpy()
                    row["ref_GiBps"] = round(m / GiB / dt, 3)
                    row["equals_reference"] = bool(np.array_equal(out, mine))
                    ok = ok and row["equals_reference"]
                ok = ok and round_trip
                rows.append(row)
                print(json.dumps(row), flush=True)
            del ws
        del src
        torch.cuda.empty_cache()
    lines = [f"# mmtf / bitmmtf on the GPU ({args.gib:g} GiB device resident, median of {reps} timed enqueues after 2 warm-ups, HIP events)", "",
             f"build id: {hsrle.build_id()}  device: {torch.cuda.get_device_name(0)}", "",
             f"reference: compiled reference on one core of the same machine, first {m >> 20} MiB of the same bytes (also the bytes every output is compared on);",
             "copy: device-to-device copy of the same size.", "",
             "| transform | direction | input | GPU ms | GPU GiB/s | reference 1 core GiB/s | GPU / reference | copy GiB/s | equals reference | round trip |",
             "|---|---|---|---:|---:|---:|---:|---:|---|---|"]
    for r in rows:
        rr = r["ref_GiBps"]
        lines.append(f"| {r['transform']} | {r['direction']} | {r['input']} | {r['ms']:.3f} | {r['gpu_GiBps']:.2f} | {('%.3f' % rr) if rr else 'n/a'} | "
                     f"{('%.1f' % (r['gpu_GiBps'] / rr)) if rr else 'n/a'} | {r['copy_GiBps']:.1f} | {'n/a' if r['equals_reference'] is None else ('yes' if r['equals_reference'] else 'NO')} | "
                     f"{'yes' if r['round_trip'] else 'NO'} |")
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
