#!/usr/bin/env python3
"""Device time of the rle8_mmtf128 checkpoints and byte-range decode (include/hsrle.h section 5) next to the whole indexed decode, on device-resident data:
the three inputs of tools/rle8_mmtf_time.py (video-shaped and run-distributed hsrle_synth_dev bytes, and the stream of many tiny packets).

Per size and input, medians of --reps timed enqueues (HIP events) in ONE run:
  * hsrle_rle8_mmtf128_decompress_indexed_dev_async of the whole stream,
  * hsrle_rle8_mmtf128_checkpoints_build_dev_async at every checkpointRows of --checkpoint-rows, and the sidecar's share of stream and input,
  * hsrle_rle8_mmtf128_decompress_range_dev_async of --ranges KiB at the start, in the middle and at the end of the stream, at every checkpointRows.
The middle range starts one byte behind a checkpoint row's middle, so that it pays about half a checkpoint spacing of rows in front of it; the end range
ends with the stream.  Checks: every status word, the sidecar's header against hsrle_rle8_mmtf128_checkpoints_bound, every decode and every range against
the input (torch.equal on the device).
Per-kernel times: the same command with --once under a kernel trace: every new kernel then runs once per row after one warm-up.

  python tools/rle8_mmtf_range_time.py [--mib 64,1024] [--reps 5] [--spacing 1024] [--checkpoint-rows 16384,65536,262144] [--ranges 64,1024,16384]
                                       [--out profiles/r19_rle8_mmtf_range.md]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hypersonic-rle-kit_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import torch  # noqa: E402
import hsrle  # noqa: E402
from rle8_mmtf_time import timed, tiny_packets  # noqa: E402


def median_ms(fn, reps, warm):
    timed(fn)
    return statistics.median([timed(fn) for _ in range(reps + warm - 1)][-reps:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="64,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spacing", type=int, default=1024)
    ap.add_argument("--checkpoint-rows", default="16384,65536,262144")
    ap.add_argument("--ranges", default="64,1024,16384", help="range lengths in KiB")
    ap.add_argument("--inputs", default="video,runs,tiny_packets")
    ap.add_argument("--once", action="store_true", help="one warm-up and one timed enqueue per row (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps, warm = (1, 1) if args.once else (max(args.reps, 3), 2)
    ck_list = [int(s) for s in args.checkpoint_rows.split(",")]
    lengths = [int(s) << 10 for s in args.ranges.split(",")]
    hsrle.mmtf_tuning(0)
    hsrle.rle8_mmtf_tuning(0)
    default_ck = (1 << 30) // 16 // ((hsrle.rle8_mmtf128_checkpoints_bound(1 << 30, 0) - 64) // 4096 + 1)
    builds, rows, ok = [], [], True
    for mib in (int(m) for m in args.mib.split(",")):
        n = min(mib << 20, 1 << 30)
        enc = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        dec = torch.empty(n, dtype=torch.uint8, device="cuda")
        out = torch.empty(max(min(l, n) for l in lengths), dtype=torch.uint8, device="cuda")
        words = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        sizes = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        wsc = torch.full((hsrle.rle8_mmtf128_workspace_size(0, n),), 0xC3, dtype=torch.uint8, device="cuda")
        wsd = torch.full((hsrle.rle8_mmtf128_workspace_size(1, n),), 0xC3, dtype=torch.uint8, device="cuda")
        index = torch.empty(hsrle.rle8_mmtf128_index_bound(n, args.spacing), dtype=torch.uint8, device="cuda")
        for kname in args.inputs.split(","):
            src = tiny_packets(n) if kname == "tiny_packets" else hsrle.synth(hsrle.SYNTH_VIDEO if kname == "video" else hsrle.SYNTH_RUNS, 1, 2, n, device="cuda")
            hsrle.rle8_mmtf128_compress_indexed_dev(src, enc, words[0:1], words[1:2], wsc, index, sizes[0:1], spacing_rows=args.spacing)
            torch.cuda.synchronize()
            size, isz = int(words[0].item()), int(sizes[0].item())
            if int(words[1].item()) != hsrle.RLE8_MMTF_DONE or isz < 64:
                sys.exit(f"{kname}: compress_indexed status {int(words[1].item())}")
            stream = enc[:size]
            info = hsrle.rle8_mmtf128_index_info(index[:64].cpu().numpy().tobytes() + bytes(isz - 64))
            dec.zero_()
            whole = median_ms(lambda: hsrle.rle8_mmtf128_decompress_indexed_dev(stream, index[:isz], info, dec, words[2:3], wsd), reps, warm)
            torch.cuda.synchronize()
            ok = ok and int(words[2].item()) == hsrle.RLE8_MMTF_DONE and bool(torch.equal(dec, src))
            for ck_rows in ck_list:
                bound = hsrle.rle8_mmtf128_checkpoints_bound(n, ck_rows)
                side = torch.empty(bound, dtype=torch.uint8, device="cuda")
                build = median_ms(lambda: hsrle.rle8_mmtf128_checkpoints_build_dev(stream, index[:isz], info, side, sizes[1:2], words[3:4], wsd, checkpoint_rows=ck_rows), reps, warm)
                torch.cuda.synchronize()
                good = int(words[3].item()) == hsrle.RLE8_MMTF_DONE and int(sizes[1].item()) == bound
                ck = hsrle.rle8_mmtf128_checkpoints_info(side[:64].cpu().numpy().tobytes() + bytes(bound - 64)) if good else None
                good = good and (ck.checkpointRows, ck.uncompressedSize, ck.streamSize, ck.size) == (ck_rows, n, size, bound)
                ok = ok and good
                row = {"mib": n >> 20, "input": kname, "checkpoint_rows": ck_rows, "stream_bytes": size, "sidecar_bytes": bound, "decompress_indexed_ms": whole,
                       "checkpoints_build_ms": build, "checks": good}
                builds.append(row)
                print(json.dumps(row), flush=True)
                if not good:
                    continue
                for length in sorted({min(l, n) for l in lengths}):
                    ws = torch.full((hsrle.rle8_mmtf128_range_workspace_size(length, args.spacing, ck_rows),), 0xC3, dtype=torch.uint8, device="cuda")
                    middle = min((n // 2 // (16 * ck_rows)) * 16 * ck_rows + 8 * ck_rows + 1, n - length)
                    for where, offset in (("start", 0), ("middle", middle), ("end", n - length)):
                        dst = out[:length]
                        dst.zero_()
                        ms = median_ms(lambda: hsrle.rle8_mmtf128_decompress_range_dev(stream, index[:isz], info, side, ck, offset, length, dst, words[2:3], ws), reps, warm)
                        torch.cuda.synchronize()
                        good = int(words[2].item()) == hsrle.RLE8_MMTF_DONE and bool(torch.equal(dst, src[offset : offset + length]))
                        ok = ok and good
                        row = {"mib": n >> 20, "input": kname, "checkpoint_rows": ck_rows, "range_kib": length >> 10, "where": where, "offset": offset,
                               "workspace_bytes": ws.numel(), "range_ms": ms, "decompress_indexed_ms": whole, "checks": good}
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                    del ws
                del side
            del src
            torch.cuda.empty_cache()
        del enc, dec, out, wsc, wsd, index
        torch.cuda.empty_cache()
    lines = [f"# rle8_mmtf128 checkpoints and byte-range decode on the GPU (device resident, median of {reps} timed enqueues, HIP events)", "",
             f"build id: {hsrle.build_id()}  device: {torch.cuda.get_device_name(0)}  index spacing: {args.spacing} rows  default checkpointRows: {default_ck}", "",
             "## checkpoints_build beside decompress_indexed of the same stream", "",
             "| MiB | input | checkpointRows | sidecar bytes | sidecar / stream | sidecar / input | decompress_indexed ms | checkpoints_build ms | build / indexed | checks |",
             "|---:|---|---:|---:|---:|---:|---:|---:|---:|---|"]
    for r in builds:
        lines.append(f"| {r['mib']} | {r['input']} | {r['checkpoint_rows']} | {r['sidecar_bytes']} | {r['sidecar_bytes'] / r['stream_bytes']:.5f} | "
                     f"{r['sidecar_bytes'] / (r['mib'] << 20):.5f} | {r['decompress_indexed_ms']:.3f} | {r['checkpoints_build_ms']:.3f} | "
                     f"{r['checkpoints_build_ms'] / r['decompress_indexed_ms']:.2f} | {'yes' if r['checks'] else 'NO'} |")
    lines += ["", "## decompress_range beside decompress_indexed of the whole stream", "",
              "| MiB | input | checkpointRows | range KiB | where | workspace MiB | range ms | whole indexed ms | whole / range | checks |", "|---:|---|---:|---:|---|---:|---:|---:|---:|---|"]
    for r in rows:
        lines.append(f"| {r['mib']} | {r['input']} | {r['checkpoint_rows']} | {r['range_kib']} | {r['where']} | {r['workspace_bytes'] / (1 << 20):.2f} | {r['range_ms']:.3f} | "
                     f"{r['decompress_indexed_ms']:.3f} | {r['decompress_indexed_ms'] / r['range_ms']:.1f} x | {'yes' if r['checks'] else 'NO'} |")
    slower = [r for r in rows if r["range_kib"] == 1024 and r["range_ms"] >= r["decompress_indexed_ms"]]
    lines += ["", f"1 MiB ranges that are not faster than the whole indexed decode of the same run: {len(slower)} of {sum(r['range_kib'] == 1024 for r in rows)}"]
    lines += [f"- {r['mib']} MiB {r['input']} checkpointRows {r['checkpoint_rows']} {r['where']}: {r['range_ms']:.3f} ms against {r['decompress_indexed_ms']:.3f} ms" for r in slower]
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
