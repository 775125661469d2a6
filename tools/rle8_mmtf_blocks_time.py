#!/usr/bin/env python3
"""Device time of the rle8_mmtf128 block container (hsrle_rle8_mmtf128_compress_blocks_dev_async / _decompress_blocks_dev_async), both directions, on
device-resident data: run-distributed and video-shaped hsrle_synth_dev bytes, and random bytes -- after tools/rle8_sh_blocks_time.py.

Per size (--mib, default 64 and 1024), input and block size (--blocks, default 1024, 4096, 16384, 65536): the median of --reps timed enqueues (HIP
events, 2 warm-ups).  Beside the rows of --single-mib MiB (default 64): the SINGLE-STREAM call of the same library (hsrle_rle8_mmtf128_compress_dev_async /
_decompress_dev_async) on the same bytes, one timed enqueue after one warm-up (a decompress enqueue takes up to seconds), and how much the container
grows over that one stream: every block pays 8 header bytes and a terminator, its runs end at its edges, and its move-to-front lists restart as the
identity, so every symbol of a block is ranked by its VALUE the first time a column sees it.
Checks: the device status words, decompress(compress(x)) == x on the device for the whole buffer, and that the first and the last block stream of
every container equal the single-stream encoder's stream of those bytes (and, with oracle/_ref/libhsrle_ref.so, the compiled reference's behind the
first COPY packet, whose width the reference leaves to an undefined start value).
Per-kernel times: run the same command with --once under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/rle8_mmtf_blocks_time.py
--once --mib 64 --blocks 4096 --no-single): every kernel then runs once per group, input and direction, after one warm-up.

  python tools/rle8_mmtf_blocks_time.py [--mib 64,1024] [--blocks 1024,4096,16384,65536] [--reps 5] [--out profiles/r17_rle8_mmtf_blocks.md]
"""
import argparse
import json
import os
import statistics
import struct
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hypersonic-rle-kit_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402
import hsrle  # noqa: E402
import rle8_mmtf_testlib as T  # noqa: E402

GiB = float(1 << 30)


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


def make_input(kind, n):
    if kind == "random":
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    return hsrle.synth(hsrle.SYNTH_VIDEO if kind == "video" else hsrle.SYNTH_RUNS, 1, 2, n, device="cuda")


def single_stream(src, reps, warm):
    """(stream bytes, compress ms, decompress ms, round trip) of the single-stream call on `src`."""
    n = src.numel()
    enc = torch.empty(n + 13, dtype=torch.uint8, device="cuda")
    dec = torch.empty(n, dtype=torch.uint8, device="cuda")
    words = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    wsc = torch.full((hsrle.rle8_mmtf128_workspace_size(0, n),), 0xC3, dtype=torch.uint8, device="cuda")
    wsd = torch.full((hsrle.rle8_mmtf128_workspace_size(1, n),), 0xC3, dtype=torch.uint8, device="cuda")
    c = median_ms(lambda: hsrle.rle8_mmtf128_compress_dev(src, enc, words[0:1], words[1:2], wsc), reps, warm)[0]
    size = int(words[0].item())
    if int(words[1].item()) != hsrle.RLE8_MMTF_DONE:
        sys.exit("single stream: compress failed")
    d = median_ms(lambda: hsrle.rle8_mmtf128_decompress_dev(enc[:size], dec, words[2:3], wsd), reps, warm)[0]
    ok = int(words[2].item()) == hsrle.RLE8_MMTF_DONE and bool(torch.equal(dec, src))
    return size, c, d, ok


def block_streams_agree(src, container, info, ref):
    """The first and the last block stream against the single-stream encoder (and the compiled reference) on those bytes."""
    head = container[: info.payload_start].cpu().numpy().tobytes()
    off = struct.unpack_from(f"<{info.blockCount + 1}Q", head, 64)
    for i in sorted({0, info.blockCount - 1}):
        block = src[i * info.blockSize : min((i + 1) * info.blockSize, src.numel())].cpu().numpy().tobytes()
        mine = container[info.payload_start + off[i] : info.payload_start + off[i + 1]].cpu().numpy().tobytes()
        size, theirs = hsrle.rle8_mmtf128_compress(block, out_cap=len(block) + 13)
        if size == 0 or mine != theirs:
            return False
        if ref is not None:
            r = ref.compress(block)
            if mine[T.first_copy_end(mine) :] != r[T.first_copy_end(r) :] or ref.decompress(mine, len(block)) != (len(block), block):
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", default="64,1024")
    ap.add_argument("--blocks", default="1024,4096,16384,65536")
    ap.add_argument("--inputs", default="runs,video,random")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single-mib", type=int, default=64)
    ap.add_argument("--no-single", action="store_true")
    ap.add_argument("--in-flight", type=int, default=0, help="hsrle_rle8_mmtf128_blocks_tuning (0 = the default)")
    ap.add_argument("--once", action="store_true", help="one warm-up and one timed enqueue per row (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    reps, warm = (1, 1) if args.once else (max(args.reps, 3), 2)
    ref = T.Rle8MmtfReference() if T.Rle8MmtfReference.available() else None
    hsrle.rle8_mmtf_tuning(0)
    hsrle.mmtf_tuning(0)
    hsrle.rle8_mmtf128_blocks_tuning(args.in_flight)
    rows, singles, ok = [], [], True
    for mib in (int(x) for x in args.mib.split(",")):
        n = mib << 20
        for kind in args.inputs.split(","):
            src = make_input(kind, n)
            single = None
            if mib == args.single_mib and not args.no_single:
                size, c, d, good = single_stream(src, 1, 1)
                single = {"input": kind, "bytes": n, "stream_bytes": size, "compress_ms": round(c, 3), "decompress_ms": round(d, 3), "round_trip": good}
                singles.append(single)
                ok = ok and good
                print(json.dumps(single), flush=True)
                torch.cuda.empty_cache()
            dec = torch.empty(n, dtype=torch.uint8, device="cuda")
            for bs in (int(x) for x in args.blocks.split(",")):
                enc = torch.empty(hsrle.rle8_mmtf128_blocks_bound(n, bs), dtype=torch.uint8, device="cuda")
                wsc = torch.full((hsrle.rle8_mmtf128_blocks_workspace_size(0, n, bs),), 0xC3, dtype=torch.uint8, device="cuda")
                wsd = torch.full((hsrle.rle8_mmtf128_blocks_workspace_size(1, n, bs),), 0xC3, dtype=torch.uint8, device="cuda")
                total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
                words = torch.full((2,), -1, dtype=torch.int32, device="cuda")
                hsrle.rle8_mmtf128_blocks_compress_dev(src, enc, total, words[0:1], wsc, block_size=bs)
                torch.cuda.synchronize()
                if int(words[0].item()) != hsrle.RLE8_MMTF_DONE:
                    sys.exit(f"{kind} / {bs}: compress status {int(words[0].item())}")
                container = enc[: int(total.item())]
                info = hsrle.rle8_mmtf128_blocks_info(container)
                dec.zero_()
                hsrle.rle8_mmtf128_blocks_decompress_dev(container, info, dec, words[1:2], wsd)
                torch.cuda.synchronize()
                round_trip = int(words[1].item()) == hsrle.RLE8_MMTF_DONE and bool(torch.equal(dec, src))
                agree = block_streams_agree(src, container, info, ref)
                ok = ok and round_trip and agree
                for decode in (0, 1):
                    if decode:
                        med, lo, hi = median_ms(lambda: hsrle.rle8_mmtf128_blocks_decompress_dev(container, info, dec, words[1:2], wsd), reps, warm)
                    else:
                        med, lo, hi = median_ms(lambda: hsrle.rle8_mmtf128_blocks_compress_dev(src, enc, total, words[0:1], wsc, block_size=bs), reps, warm)
                    base = None if single is None else single["decompress_ms" if decode else "compress_ms"]
                    row = {"direction": "decompress" if decode else "compress", "input": kind, "bytes": n, "block_size": bs, "blocks": info.blockCount,
                           "container_bytes": info.totalSize, "ms": round(med, 3), "spread_ms": [round(lo, 3), round(hi, 3)], "GiBps": round(n / GiB / (med / 1e3), 2),
                           "single_stream_ms": base, "single_stream_bytes": None if single is None else single["stream_bytes"],
                           "workspace_bytes": (wsd if decode else wsc).numel(), "round_trip": round_trip, "block_streams_agree": agree}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del enc, wsc, wsd, container
                torch.cuda.empty_cache()
            del src, dec
            torch.cuda.empty_cache()
    lines = [f"# The rle8_mmtf128 block container on the GPU (device resident, median of {reps} timed enqueues after {warm} warm-ups, HIP events)", "",
             f"build id: {hsrle.build_id()}  device: {torch.cuda.get_device_name(0)}  blocks in flight: {args.in_flight or 'default'}", "",
             "`single stream`: hsrle_rle8_mmtf128_compress_dev_async / _decompress_dev_async of the same library on the same bytes, one timed enqueue after one warm-up.",
             "`agree`: the first and the last block stream equal the single-stream encoder's" + (" and, behind the first COPY packet, the compiled reference's" if ref else "") + " stream of those bytes.", "",
             "| MiB | input | block | direction | container / input | ms | GiB/s | single stream ms | speed-up | container / single stream | workspace MiB | round trip | agree |",
             "|---:|---|---:|---|---:|---:|---:|---:|---:|---:|---:|---|---|"]
    for r in rows:
        s = r["single_stream_ms"]
        lines.append(f"| {r['bytes'] >> 20} | {r['input']} | {r['block_size']} | {r['direction']} | {r['container_bytes'] / r['bytes']:.4f} | {r['ms']:.3f} | {r['GiBps']:.2f} | "
                     f"{('%.3f' % s) if s else 'n/a'} | {(('%.0f x' if s / r['ms'] >= 10 else '%.2f x') % (s / r['ms'])) if s else 'n/a'} | "
                     f"{('%.4f' % (r['container_bytes'] / r['single_stream_bytes'])) if r['single_stream_bytes'] else 'n/a'} | {r['workspace_bytes'] / (1 << 20):.1f} | "
                     f"{'yes' if r['round_trip'] else 'NO'} | {'yes' if r['block_streams_agree'] else 'NO'} |")
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
