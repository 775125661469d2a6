#!/usr/bin/env python3
"""The span algebra of the rle8_mmtf128 encoder (csrc/hsrle_rle8mmtf.hip.h: k_rm_classify, k_rm_scan, k_rm_emit) stated on the CPU, pass by pass and
with the kernels' own per-span tables, so that it can be held against the sequential model (tests/rle8_mmtf_testlib.py) without a GPU:
  classify  per span of SP rows: starts, first / last start, OR in front of the first start, OR behind the last start, bytes of the closed packets
  scan      a suffix sweep closes every open packet (count, OR), a prefix sweep gives every span its stream offset and the span its incoming packet began in
  emit      every span writes the headers of the packets that begin in it and the bodies of its rows; a group is written by the span of its first row
`threads` cuts the scan into runs of spans with a hand-over between them, as the kernel's 1 024 threads do.

  python tools/rle8_mmtf_span_model.py          # self-check on random inputs
"""
import os
import struct
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import rle8_mmtf_testlib as T  # noqa: E402
from mmtf_testlib import mmtf_enc  # noqa: E402

NONE = None


def row_class(row):
    return 0x100 | row[0] if T.is_uniform(row) else 0


def packet_bytes(rle, count, code):
    if rle:
        return 2 if count < 128 else 5
    return (1 if count < 32 else 4) + count * T.ROW_BYTES[code]


def classify(rows, SP):
    R = len(rows)
    spans = []
    for k in range((R + SP - 1) // SP):
        lo, hi = k * SP, min(R, k * SP + SP)
        cls = [row_class(r) for r in rows[lo:hi]]
        prev = [row_class(rows[lo - 1]) if lo else NONE] + cls[:-1]
        start = [lo + l == 0 or cls[l] != prev[l] for l in range(hi - lo)]
        lanes = [l for l in range(hi - lo) if start[l]]
        s = {"ns": len(lanes), "first": lanes[0] if lanes else 64, "last": lanes[-1] if lanes else 64, "closed": 0, "open_rle": 0, "open_pre": 0, "tail_or": 0}
        s["head_or"] = T.rows_or(rows[lo : lo + (lanes[0] if lanes else hi - lo)])
        for a, b in zip(lanes, lanes[1:] + [hi - lo]):
            rle = bool(cls[a] & 0x100)
            pre = 1 if rle and (lo + a == 0 or (prev[a] or 0) & 0x100) else 0
            if a == lanes[-1]:
                s["open_rle"], s["open_pre"], s["tail_or"] = rle, pre, T.rows_or(rows[lo + a : hi])
            else:
                s["closed"] += pre + packet_bytes(rle, b - a, T.width_code(T.rows_or(rows[lo + a : lo + b])))
        spans.append(s)
    return spans


def scan(spans, R, SP, threads):
    N = len(spans)
    per = (N + threads - 1) // threads
    runs = [(min(N, t * per), min(N, t * per + per)) for t in range(threads)]
    res = [dict(base=0, count=0, code=0, prev=NONE) for _ in range(N)]
    # suffix sweep: the summaries of the runs, the hand-over from the right, the sweep proper
    summary = []
    for lo, hi in runs:
        nsr, acc = NONE, 0
        for k in range(hi - 1, lo - 1, -1):
            s = spans[k]
            if s["ns"]:
                nsr, acc = k * SP + s["first"], s["head_or"]
            else:
                acc |= s["head_or"]
        summary.append((nsr, acc))
    incoming, n, o = [None] * threads, R, 0
    for t in range(threads - 1, -1, -1):
        incoming[t] = (n, o)
        f, g = summary[t]
        if f is not NONE:
            n, o = f, g
        else:
            o |= g
    totals = []
    for t, (lo, hi) in enumerate(runs):
        nsr, acc = incoming[t]
        total, last_ne = 0, NONE
        for k in range(hi - 1, lo - 1, -1):
            s = spans[k]
            if s["ns"]:
                r = res[k]
                r["count"] = nsr - (k * SP + s["last"])
                r["code"] = T.width_code(s["tail_or"] | acc)
                r["base"] = s["closed"] + s["open_pre"] + packet_bytes(s["open_rle"], r["count"], r["code"])
                total += r["base"]
                if last_ne is NONE:
                    last_ne = k
                nsr, acc = k * SP + s["first"], s["head_or"]
            else:
                acc |= s["head_or"]
        totals.append((total, last_ne))
    base, prev, handover = 8, NONE, []
    for total, last_ne in totals:
        handover.append((base, prev))
        base += total
        if last_ne is not NONE:
            prev = last_ne
    for t, (lo, hi) in enumerate(runs):
        b, p = handover[t]
        for k in range(lo, hi):
            n_bytes = res[k]["base"]
            res[k]["base"], res[k]["prev"] = b, p
            b += n_bytes
            if spans[k]["ns"]:
                p = k
    return res, base


def emit(rows, SP, spans, res, out):
    R = len(rows)
    for k, (s, r) in enumerate(zip(spans, res)):
        lo, hi = k * SP, min(R, k * SP + SP)
        cls = [row_class(x) for x in rows[lo:hi]]
        prev_cls = row_class(rows[lo - 1]) if lo else NONE
        off = r["base"]
        packet = None                                  # (first row, count, code, rle, body offset) of the lane's packet
        if s["first"] != 0:
            p = r["prev"]
            sp, rp = spans[p], res[p]
            o = rp["base"] + sp["closed"]
            hdr = (2 if rp["count"] < 128 else 5) if sp["open_rle"] else (1 if rp["count"] < 32 else 4)
            packet = (p * SP + sp["last"], rp["count"], rp["code"], sp["open_rle"], o + sp["open_pre"] + hdr)
        for l in range(hi - lo):
            row = lo + l
            before = cls[l - 1] if l else prev_cls
            if row == 0 or cls[l] != before:
                rle = bool(cls[l] & 0x100)
                pre = 1 if rle and (row == 0 or (before or 0) & 0x100) else 0
                if l == s["last"]:
                    count, code = r["count"], r["code"]
                else:
                    nxt = next(m for m in range(l + 1, hi - lo + 1) if m == hi - lo or cls[m] != cls[m - 1])
                    count, code = nxt - l, T.width_code(T.rows_or(rows[row : lo + nxt]))
                if pre:
                    out[off] = 0x06 if row == 0 else 0
                h = off + pre
                if rle:
                    head = bytes([count << 1, cls[l] & 0xFF]) if count < 128 else struct.pack("<IB", count << 1 | 1, cls[l] & 0xFF)
                else:
                    head = bytes([count << 3 | code << 1]) if count < 32 else struct.pack("<I", count << 3 | 1 | code << 1)
                out[h : h + len(head)] = head
                packet = (row, count, code, rle, h + len(head))
                off += pre + packet_bytes(rle, count, code)
            first, count, code, rle, body = packet
            if rle:
                continue
            i = row - first
            G = {0: 1, 1: 2, 2: 6, 3: 4}[code]
            full = count // G * G
            if i < full:
                if i % G == 0:                         # the lane of the group's first row writes the group (its rows may lie in the next span)
                    b = T.pack_rows(rows[row : row + G], code)
                    out[body + i * T.ROW_BYTES[code] : body + i * T.ROW_BYTES[code] + len(b)] = b
            else:                                      # a remaining row: packed alone, as a packet of one row
                b = T.pack_rows([rows[row]], code)
                out[body + i * T.ROW_BYTES[code] : body + i * T.ROW_BYTES[code] + len(b)] = b


def compress(data, SP=64, threads=1024):
    data = bytes(data)
    ranks = mmtf_enc(data, 16)
    R = len(data) // 16
    rows = [ranks[16 * i : 16 * i + 16] for i in range(R)]
    spans = classify(rows, SP)
    res, at = scan(spans, R, SP, threads)
    last_rle = R != 0 and T.is_uniform(rows[-1])
    end = 2 if R == 0 or last_rle else 1
    tail = ranks[16 * R :]
    out = bytearray(b"\xEE" * (at + end + len(tail)))
    out[0:8] = struct.pack("<II", len(data), len(out))
    out[at] = 0x06 if R == 0 else 0
    if end == 2:
        out[at + 1] = 0
    out[at + end :] = tail
    emit(rows, SP, spans, res, out)
    return bytes(out)


def main():
    n = 0
    for alphabet in (1, 2, 3, 5, 17, 256):
        for size in (1, 16, 17, 700, 5000):
            data = T.random_alphabet(size, alphabet, 7, run=2)
            want = T.model_compress(data)
            for SP, threads in ((64, 1024), (63, 3), (7, 2), (1, 5)):
                assert compress(data, SP, threads) == want, (alphabet, size, SP, threads)
                n += 1
    print(f"{n} streams equal the sequential model's")


if __name__ == "__main__":
    main()
