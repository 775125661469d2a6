#!/usr/bin/env python3
"""Device time of the rle8_mmtf128 entry index (include/hsrle.h section 5) next to the plain calls, on device-resident data: the three inputs of
tools/rle8_mmtf_time.py (video-shaped and run-distributed hsrle_synth_dev bytes, and the stream of many tiny packets).

Per size and input, medians of --reps timed enqueues (HIP events) in ONE run:
  * hsrle_rle8_mmtf128_decompress_dev_async against hsrle_rle8_mmtf128_decompress_indexed_dev_async at every spacing of --spacings,
  * hsrle_rle8_mmtf128_compress_dev_async against hsrle_rle8_mmtf128_compress_indexed_dev_async,
  * hsrle_rle8_mmtf128_index_build_dev_async (one serial walk),
  * the index's size as a share of the stream.
Checks: every status word, the stream of compress_indexed against the plain compress's, the built index against the encoder's, every decode against the
input (torch.equal on the device).  A call that takes more than a second is warmed up once, not twice.
Per-kernel times: the same command with --once --no-plain under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/rle8_mmtf_index_time.py
--once --no-plain ...): every new kernel then runs once per input, spacing and direction after one warm-up.

  python tools/rle8_mmtf_index_time.py [--mib 64,1024] [--reps 5] [--spacings 256,1024,4096] [--out profiles/r18_rle8_mmtf_index.md]
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
    first = timed(fn)
    t = [timed(fn) for _ in range(reps + (0 if first > 1000.0 or warm < 2 else warm - 1))][-reps:]
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="64,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spacings", default="256,1024,4096")
    ap.add_argument("--inputs", default="video,runs,tiny_packets")
    ap.add_argument("--once", action="store_true", help="one warm-up and one timed enqueue per row (for a kernel trace)")
    ap.add_argument("--no-plain", action="store_true", help="leave the plain decompress and the serial index build out (seconds each at 1 GiB)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps, warm = (1, 1) if args.once else (max(args.reps, 3), 2)
    spacings = [int(s) for s in args.spacings.split(",")]
    hsrle.mmtf_tuning(0)
    hsrle.rle8_mmtf_tuning(0)
    default_rows = (hsrle.rle8_mmtf128_index_bound(16 << 20, 0) - 64) // 16
    default_spacing = next(s for s in (64 << k for k in range(15)) if ((1 << 20) - 1) // s == default_rows)
    rows, ok = [], True
    for mib in (int(m) for m in args.mib.split(",")):
        n = min(mib << 20, 1 << 30)
        enc = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        enc2 = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
        dec = torch.empty(n, dtype=torch.uint8, device="cuda")
        words = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        isize = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        wsc = torch.full((hsrle.rle8_mmtf128_workspace_size(0, n),), 0xC3, dtype=torch.uint8, device="cuda")
        wsd = torch.full((hsrle.rle8_mmtf128_workspace_size(1, n),), 0xC3, dtype=torch.uint8, device="cuda")
        cap = hsrle.rle8_mmtf128_index_bound(n, min(spacings))
        index = torch.empty(cap, dtype=torch.uint8, device="cuda")
        built = torch.empty(cap, dtype=torch.uint8, device="cuda")
        for kname in args.inputs.split(","):
            src = tiny_packets(n) if kname == "tiny_packets" else hsrle.synth(hsrle.SYNTH_VIDEO if kname == "video" else hsrle.SYNTH_RUNS, 1, 2, n, device="cuda")
            plain_c = median_ms(lambda: hsrle.rle8_mmtf128_compress_dev(src, enc, words[0:1], words[1:2], wsc), reps, warm)
            torch.cuda.synchronize()
            size, status = int(words[0].item()), int(words[1].item())
            if status != hsrle.RLE8_MMTF_DONE:
                sys.exit(f"{kname}: compress status {status}")
            stream = enc[:size]
            plain_d = None
            if not args.no_plain:
                plain_d = median_ms(lambda: hsrle.rle8_mmtf128_decompress_dev(stream, dec, words[2:3], wsd), reps, warm)
                torch.cuda.synchronize()
                ok = ok and int(words[2].item()) == hsrle.RLE8_MMTF_DONE and bool(torch.equal(dec, src))
            for spacing in spacings:
                indexed_c = median_ms(lambda: hsrle.rle8_mmtf128_compress_indexed_dev(src, enc2, words[0:1], words[1:2], wsc, index, isize[0:1], spacing_rows=spacing), reps, warm)
                torch.cuda.synchronize()
                isz = int(isize[0].item())
                good = int(words[1].item()) == hsrle.RLE8_MMTF_DONE and int(words[0].item()) == size and bool(torch.equal(enc2[:size], stream)) and isz >= 64
                info = hsrle.rle8_mmtf128_index_info(index[:64].cpu().numpy().tobytes() + bytes(isz - 64)) if good else None
                good = good and (info.spacing, info.uncompressedSize, info.compressedSize, info.indexBytes) == (spacing, n, size, isz)
                build = None
                if good and not args.no_plain and spacing == default_spacing:
                    build = median_ms(lambda: hsrle.rle8_mmtf128_index_build_dev(stream, n, built, isize[1:2], words[3:4], spacing_rows=spacing), reps, warm)
                    torch.cuda.synchronize()
                    good = int(words[3].item()) == hsrle.RLE8_MMTF_DONE and int(isize[1].item()) == isz and bool(torch.equal(built[:isz], index[:isz]))
                indexed_d = None
                if good:
                    dec.zero_()
                    indexed_d = median_ms(lambda: hsrle.rle8_mmtf128_decompress_indexed_dev(stream, index[:isz], info, dec, words[2:3], wsd), reps, warm)
                    torch.cuda.synchronize()
                    good = int(words[2].item()) == hsrle.RLE8_MMTF_DONE and bool(torch.equal(dec, src))
                ok = ok and good
                row = {"mib": n >> 20, "input": kname, "spacing": spacing, "stream_bytes": size, "index_bytes": isz, "entries": (isz - 64) // 16, "decompress_ms": plain_d,
                       "decompress_indexed_ms": indexed_d, "compress_ms": plain_c, "compress_indexed_ms": indexed_c, "index_build_ms": build, "checks": good}
                rows.append(row)
                print(json.dumps(row), flush=True)
            del src
            torch.cuda.empty_cache()
        del enc, enc2, dec, wsc, wsd, index, built
        torch.cuda.empty_cache()
    f3 = lambda v: "n/a" if v is None else f"{v:.3f}"
    lines = [f"# The rle8_mmtf128 entry index on the GPU (device resident, median of {reps} timed enqueues, HIP events)", "",
             f"build id: {hsrle.build_id()}  device: {torch.cuda.get_device_name(0)}  default spacing: {default_spacing} rows", "",
             "| MiB | input | spacing rows | entries | index / stream | decompress ms | indexed ms | speed-up | compress ms | compress_indexed ms | over plain | index_build ms | checks |",
             "|---:|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---|"]
    for r in rows:
        up = "n/a" if r["decompress_ms"] is None or r["decompress_indexed_ms"] is None else f"{r['decompress_ms'] / r['decompress_indexed_ms']:.1f} x"
        lines.append(f"| {r['mib']} | {r['input']} | {r['spacing']} | {r['entries']} | {r['index_bytes'] / r['stream_bytes']:.5f} | {f3(r['decompress_ms'])} | {f3(r['decompress_indexed_ms'])} | "
                     f"{up} | {f3(r['compress_ms'])} | {f3(r['compress_indexed_ms'])} | {r['compress_indexed_ms'] / r['compress_ms']:.3f} | {f3(r['index_build_ms'])} | "
                     f"{'yes' if r['checks'] else 'NO'} |")
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
