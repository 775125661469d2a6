// hsrle_rle8mmtf.hip.h -- the rle8_mmtf128 codec of the reference (src/rle8_mmtf.c, src/rle.h:442-452) for gfx950: the mmtf128 transform
// (hsrle_mmtf.hip.h, reused as it is), run-length coding over the 16-byte rank rows, 2 / 3 / 4 bit packing of the literal rows.
//
// Stream: u32 inSize, u32 streamSize, then COPY and RLE packets in turn (COPY first), then the inSize % 16 tail ranks.  With R = inSize / 16
// rows, a row is UNIFORM when its 16 ranks are equal.  The reference's state machine reduces to a rule without carried state:
//   RLE packets  = the maximal runs of uniform rows of one rank          header c << 1, rank (c < 128) or u32 c << 1 | 1, rank
//   COPY packets = the maximal runs of non-uniform rows                   header c << 3 | flags (c < 32) or u32 c << 3 | 1 | flags
//   a null COPY 0x00 between two adjacent RLE packets; the chain starts with a COPY (count 0, byte 0x06, if row 0 is uniform or R == 0);
//   it ends with a null RLE 0x00 behind a last COPY, with a null COPY and a null RLE behind a last RLE.
// flags bits 1-2 = the WIDTH CODE of the body: 0 = 8 bit rows, 1 = 4 bit (8 bytes a row), 2 = 3 bit (6), 3 = 2 bit (4): the narrowest the OR of
// the packet's rows allows.  (The reference ORs an undefined start value into the FIRST packet's decision; here it is zero, include/hsrle.h.)
//
// Encode: ranks -> workspace (mmtf128 encode plan); then, a SPAN being `SP` <= 64 consecutive rows, one row per lane,
//   k_rm_classify  a wave per span: packet starts by neighbour comparison, a segmented OR inside the wave; leaves per span the number of
//                  starts, the first / last start, the OR of the rows in front of the first start (they belong to a packet that began in an
//                  earlier span), the OR behind the last start (that packet is OPEN: it may go on for many spans) and the bytes of the
//                  packets that begin and end inside the span
//   k_rm_scan      one workgroup, a run of spans per thread: a suffix pass closes every open packet (count and OR are reductions over the
//                  whole packet), a prefix pass gives every span the stream offset of its first packet and the span its incoming packet began
//                  in; thread 0 writes the chain's end, the tail ranks, the header, the size word and the status
//   k_rm_emit      a wave per span writes the headers of the packets that begin in it and the bodies of the rows in it.  A row's place comes
//                  from its packet's first row; a 2 / 3 / 4 bit group is written by the lane that holds its first row, which reads the other
//                  rows of the group from the rank buffer (they may lie in the next span).
// Decode:
//   k_rm_walk      ONE wave follows the header chain (the format's one serial dependence), the stream staged through LDS in 1 KiB windows,
//                  the next window in flight; one record per non-null packet (body offset, first row, count, width code / rank); verdict
//                  MALFORMED before anything is written if a packet would pass streamSize or row R or the chain has not ended at row R
//   k_rm_expand    a wave per 64 rows: search in the record list, unpack / splat into the rank buffer; the tail ranks behind them
//   then the mmtf128 decode plan from the rank buffer to the output.
#pragma once

#include "hsrle_common.hip.h"

namespace hsrle {

constexpr uint32_t kRmDone = 0u, kRmMalformed = 1u, kRmCapacity = 2u;   // == HSRLE_RLE8_MMTF_* (include/hsrle.h)
constexpr uint32_t kRmNone = 0xFFFFFFFFu;
constexpr uint32_t kRmScanThreads = 1024u;

__device__ __forceinline__ uint32_t rm_row_or(u32x4 v)
{
  uint32_t x = v[0] | v[1] | v[2] | v[3];
  x |= x >> 16;
  x |= x >> 8;
  return x & 0xFFu;
}
// 0x100 | rank for a uniform row, 0 for any other
__device__ __forceinline__ uint32_t rm_row_class(u32x4 v)
{
  const uint32_t s = (v[0] & 0xFFu) * 0x01010101u;
  return (v[0] == s && v[1] == s && v[2] == s && v[3] == s) ? (0x100u | (v[0] & 0xFFu)) : 0u;
}
// the reference's order: hi-4, then hi-6, then hi-5 (rle8_mmtf.c:257-288)
__device__ __forceinline__ uint32_t rm_width_code(uint32_t orb)
{
  if (orb & 0xF0u) return 0u;
  if ((orb & 0xFCu) == 0u) return 3u;
  return (orb & 0xF8u) == 0u ? 2u : 1u;
}
__device__ __forceinline__ uint32_t rm_row_bytes(uint32_t code) { return code == 0u ? 16u : (code == 1u ? 8u : (code == 2u ? 6u : 4u)); }
// header + body of one packet (without a null COPY in front of it)
__device__ __forceinline__ uint32_t rm_packet_bytes(bool rle, uint32_t count, uint32_t code)
{
  if (rle) return count < 128u ? 2u : 5u;
  return (count < 32u ? 1u : 4u) + count * rm_row_bytes(code);
}
__device__ __forceinline__ u32x4 rm_ld_row(const uint8_t *ranks, uint32_t row) { return *(const u32x4 *)__builtin_assume_aligned(ranks + (uint64_t)row * 16u, 16); }

// bit `bit` of each of the 16 bytes, byte j -> bit j (_mm_movemask_epi8 of the row shifted left by 7 - bit)
__device__ __forceinline__ uint32_t rm_movemask(u32x4 v, uint32_t bit)
{
  uint32_t m = 0;
#pragma unroll
  for (int d = 0; d < 4; d++) m |= ((((v[d] >> bit) & 0x01010101u) * 0x01020408u) >> 24 & 0xFu) << (4 * d);
  return m;
}
// the inverse: bit j of m -> bit 0 of byte j
__device__ __forceinline__ u32x4 rm_spread(uint32_t m)
{
  u32x4 v;
#pragma unroll
  for (int d = 0; d < 4; d++) v[d] = (((m >> (4 * d)) & 0xFu) * 0x00204081u) & 0x01010101u;
  return v;
}

// One span in a wave: lane l holds row span * SP + l.
struct RmSpan
{
  u32x4 v;
  uint32_t row, nvalid, cls, prevCls, segEnd, orSeg, pre;
  uint64_t M;          // lanes that start a packet
  bool valid, start, rle;
};
__device__ __forceinline__ void rm_span_load(const uint8_t *ranks, uint32_t R, uint32_t SP, uint32_t span, uint32_t lane, RmSpan &s)
{
  const uint32_t row0 = span * SP;
  s.nvalid = umin(SP, R - row0);
  s.valid = lane < s.nvalid;
  s.row = row0 + lane;
  const u32x4 zero = { 0u, 0u, 0u, 0u };
  s.v = s.valid ? rm_ld_row(ranks, s.row) : zero;
  s.cls = s.valid ? rm_row_class(s.v) : kRmNone;
  uint32_t prev = __shfl_up(s.cls, 1, 64);
  if (lane == 0u) prev = row0 != 0u ? rm_row_class(rm_ld_row(ranks, row0 - 1u)) : kRmNone;
  s.prevCls = prev;
  s.start = s.valid && (s.row == 0u || s.cls != prev);
  s.rle = (s.cls & 0x100u) != 0u;
  // a null COPY in front of an RLE packet that follows an RLE packet; the first COPY of count 0 in front of an RLE packet at row 0
  s.pre = (s.start && s.rle && (s.row == 0u || (prev & 0x100u) != 0u)) ? 1u : 0u;
  s.M = __ballot(s.start);
  const uint64_t above = lane == 63u ? 0ull : (s.M & ~((2ull << lane) - 1ull));
  s.segEnd = above ? (uint32_t)__builtin_ctzll(above) : s.nvalid;
  uint32_t x = s.valid ? rm_row_or(s.v) : 0u;   // OR of the rows from this lane to the end of its packet's part of the span
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1)
  {
    const uint32_t y = __shfl_down(x, o, 64);
    if (lane + o < s.segEnd) x |= y;
  }
  s.orSeg = x;
}
__device__ __forceinline__ uint32_t rm_wave_sum(uint32_t x)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

// per span, from k_rm_classify: x = starts | first start lane << 8 | last << 16 | open packet is RLE << 24 | has a byte in front << 25,
//                               y = OR in front of the first start | OR from the last start on << 8,  z = bytes of the closed packets
// per span, from k_rm_scan:     x = stream offset of the first packet that starts in the span, y = count of its open packet, z = its width code,
//                               w = the last span before this one in which a packet starts
// (behind k_rm_emit the entry index's k_rm_index_count reuses y and z: hsrle_rle8mmtf_index.hip.h)
struct RmEncArgs
{
  const uint8_t *ranks;   // 16-byte aligned, rows * 16 + tail bytes
  uint8_t *out;
  uint4 *sum, *res;
  uint32_t *ctrl;         // [0] = 1: the stream does not fit
  uint32_t *outSize, *status;
  uint32_t size, rows, SP, spans, outCap;
};

// The passes are __device__ functions of one wave (d_rm_scan: of one workgroup): the kernels below call them for the one stream of a call, the kernels
// of the blocked form (hsrle_rle8mmtfb.hip.h: a wave per block) for the stream of every block.
__device__ __forceinline__ void d_rm_classify(const RmEncArgs &a, uint32_t span, uint32_t lane)
{
  RmSpan s;
  rm_span_load(a.ranks, a.rows, a.SP, span, lane, s);
  const uint32_t ns = (uint32_t)__popcll(s.M);
  uint32_t first = 64u, last = 64u, closed = 0u, openRle = 0u, openPre = 0u, tailOr = 0u;
  if (ns != 0u)
  {
    first = (uint32_t)__builtin_ctzll(s.M);
    last = 63u - (uint32_t)__builtin_clzll(s.M);
    const uint32_t mine = (s.start && lane != last) ? s.pre + rm_packet_bytes(s.rle, s.segEnd - lane, rm_width_code(s.orSeg)) : 0u;
    closed = rm_wave_sum(mine);
    openRle = __shfl(s.rle ? 1u : 0u, last, 64);
    openPre = __shfl(s.pre, last, 64);
    tailOr = __shfl(s.orSeg, last, 64);
  }
  const uint32_t headOr = (first != 0u) ? __shfl(s.orSeg, 0, 64) : 0u;
  if (lane == 0u)
    a.sum[span] = make_uint4(ns | first << 8 | last << 16 | openRle << 24 | openPre << 25, headOr | tailOr << 8, closed, 0u);
}

template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_rm_classify(RmEncArgs a)
{
  const uint32_t lane = threadIdx.x & 63u, span = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (span >= a.spans) return;
  d_rm_classify(a, span, lane);
}

// A workgroup of T threads (sA, sB: T words of LDS each, sTotal: one): closes and places the packets; returns the offset behind the last packet.
template <uint32_t T>
__device__ __forceinline__ uint32_t d_rm_scan(const RmEncArgs &a, uint32_t t, uint32_t *sA, uint32_t *sB, uint32_t *sTotal)
{
  const uint32_t N = a.spans, SP = a.SP;
  const uint32_t per = (N + T - 1u) / T;
  const uint64_t lo64 = (uint64_t)t * per;
  const uint32_t lo = (uint32_t)(lo64 < N ? lo64 : N), hi = (uint32_t)(lo64 + per < N ? lo64 + per : N);
  // suffix pass: the next packet start behind a span and the OR of the rows up to it.  First the run's summary ...
  uint32_t nsr = kRmNone, acc = 0u;
  for (uint32_t k = hi; k-- > lo;)
  {
    const uint4 q = a.sum[k];
    if (q.x & 0xFFu) { nsr = k * SP + ((q.x >> 8) & 0xFFu); acc = q.y & 0xFFu; }
    else acc |= q.y & 0xFFu;
  }
  sA[t] = nsr;
  sB[t] = acc;
  __syncthreads();
  if (t == 0u)   // ... then what comes in from the right of every run
  {
    uint32_t n = a.rows, o = 0u;
    for (uint32_t i = T; i-- > 0u;)
    {
      const uint32_t f = sA[i], g = sB[i];
      sA[i] = n;
      sB[i] = o;
      if (f != kRmNone) { n = f; o = g; }
      else o |= g;
    }
  }
  __syncthreads();
  nsr = sA[t];
  acc = sB[t];
  __syncthreads();
  uint32_t bytes = 0u, lastNE = kRmNone;
  for (uint32_t k = hi; k-- > lo;)
  {
    const uint4 q = a.sum[k];
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (q.x & 0xFFu)
    {
      const bool rle = (q.x >> 24) & 1u;
      r.y = nsr - (k * SP + ((q.x >> 16) & 0xFFu));
      r.z = rm_width_code(((q.y >> 8) & 0xFFu) | acc);
      r.x = q.z + ((q.x >> 25) & 1u) + rm_packet_bytes(rle, r.y, r.z);   // (for now: the bytes of the packets that start in the span)
      bytes += r.x;
      if (lastNE == kRmNone) lastNE = k;
      nsr = k * SP + ((q.x >> 8) & 0xFFu);
      acc = q.y & 0xFFu;
    }
    else acc |= q.y & 0xFFu;
    a.res[k] = r;
  }
  sA[t] = bytes;
  sB[t] = lastNE;
  __syncthreads();
  if (t == 0u)
  {
    uint32_t base = 8u, prev = kRmNone;
    for (uint32_t i = 0; i < T; i++)
    {
      const uint32_t b = sA[i], l = sB[i];
      sA[i] = base;
      sB[i] = prev;
      base += b;
      if (l != kRmNone) prev = l;
    }
    *sTotal = base;
  }
  __syncthreads();
  uint32_t base = sA[t], prev = sB[t];
  for (uint32_t k = lo; k < hi; k++)
  {
    uint4 r = a.res[k];
    const uint32_t b = r.x;
    r.x = base;
    r.w = prev;
    a.res[k] = r;
    base += b;
    if (a.sum[k].x & 0xFFu) prev = k;
  }
  return *sTotal;
}

// the chain's end: 0x06 0x00 without a row, 0x00 behind a last COPY, 0x00 0x00 behind a last RLE
__device__ __forceinline__ uint32_t rm_chain_end(const RmEncArgs &a)
{
  const uint32_t R = a.rows;
  return (R == 0u || rm_row_class(rm_ld_row(a.ranks, R - 1u)) != 0u) ? 2u : 1u;
}
// one lane: the header, the chain's end at `at` and the tail ranks behind it; the stream's size is at + end + the tail
__device__ __forceinline__ void d_rm_close(const RmEncArgs &a, uint32_t at, uint32_t end)
{
  const uint32_t R = a.rows, tail = a.size - R * 16u;
  st32(a.out, a.size);
  st32(a.out + 4, at + end + tail);
  a.out[at] = R == 0u ? (uint8_t)0x06 : (uint8_t)0;
  if (end == 2u) a.out[at + 1u] = 0;
  for (uint32_t i = 0; i < tail; i++) a.out[at + end + i] = a.ranks[(uint64_t)R * 16u + i];
}

template <int UNUSED = 0>
__global__ __launch_bounds__(1024) void k_rm_scan(RmEncArgs a)
{
  __shared__ uint32_t sA[kRmScanThreads], sB[kRmScanThreads];
  __shared__ uint32_t sTotal;
  const uint32_t at = d_rm_scan<kRmScanThreads>(a, threadIdx.x, sA, sB, &sTotal);
  if (threadIdx.x == 0u)
  {
    const uint32_t end = rm_chain_end(a), total = at + end + (a.size - a.rows * 16u);
    const bool fits = total <= a.outCap;
    if (fits) d_rm_close(a, at, end);
    a.ctrl[0] = fits ? 0u : 1u;
    *a.outSize = fits ? total : 0u;
    *a.status = fits ? kRmDone : kRmCapacity;
  }
}

// Every store lies inside the packet it belongs to and is a whole byte, word or vector of it: nothing is read-modify-written, nothing lands behind the
// stream.  The other rows of a 2 / 3 / 4 bit group come from a.ranks, below row a.rows.
__device__ __forceinline__ void d_rm_emit(const RmEncArgs &a, uint32_t span, uint32_t lane)
{
  RmSpan s;
  rm_span_load(a.ranks, a.rows, a.SP, span, lane, s);
  const uint4 r = a.res[span];
  const uint32_t ns = (uint32_t)__popcll(s.M);
  const uint32_t last = ns ? 63u - (uint32_t)__builtin_clzll(s.M) : 64u;
  // the packets that start here: count, width code, stream offset (of the byte in front, if there is one)
  uint32_t cnt = 0u, code = 0u, bytes = 0u;
  if (s.start)
  {
    cnt = lane == last ? r.y : s.segEnd - lane;
    code = lane == last ? r.z : rm_width_code(s.orSeg);
    bytes = s.pre + rm_packet_bytes(s.rle, cnt, code);
  }
  uint32_t inc = bytes;
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1)
  {
    const uint32_t y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  uint32_t off = r.x + inc - bytes, pre = s.pre, first = s.row;
  bool rle = s.rle;
  // every lane learns its packet: from the start lane at or below it, or -- in front of the first start -- from the span the packet began in
  const uint64_t below = s.M & (lane == 63u ? ~0ull : ((2ull << lane) - 1ull));
  const uint32_t src = below ? 63u - (uint32_t)__builtin_clzll(below) : 0u;
  const uint32_t gCnt = __shfl(cnt, src, 64), gCode = __shfl(code, src, 64), gOff = __shfl(off, src, 64), gPre = __shfl(pre, src, 64), gFirst = __shfl(first, src, 64);
  if (below) { cnt = gCnt; code = gCode; off = gOff; pre = gPre; first = gFirst; }
  else if (s.valid)
  {
    const uint32_t p = r.w;        // (a span without a start in front of it does not exist: row 0 starts a packet)
    const uint4 qs = a.sum[p], qr = a.res[p];
    cnt = qr.y; code = qr.z;
    off = qr.x + qs.z;
    pre = (qs.x >> 25) & 1u;
    first = p * a.SP + ((qs.x >> 16) & 0xFFu);
    rle = (qs.x >> 24) & 1u;
  }
  if (!s.valid) return;
  uint8_t *p = a.out + off;
  if (s.start)
  {
    if (pre) p[0] = s.row == 0u ? (uint8_t)0x06 : (uint8_t)0;
    uint8_t *h = p + pre;
    if (rle)
    {
      if (cnt < 128u) { h[0] = (uint8_t)(cnt << 1); h[1] = (uint8_t)s.cls; }
      else { st32(h, cnt << 1 | 1u); h[4] = (uint8_t)s.cls; }
    }
    else if (cnt < 32u) h[0] = (uint8_t)(cnt << 3 | code << 1);
    else st32(h, cnt << 3 | 1u | code << 1);
  }
  if (rle) return;
  uint8_t *body = p + pre + (cnt < 32u ? 1u : 4u);
  const uint32_t i = s.row - first;
  const u32x4 v = s.v;
  if (code == 0u)
    st128(body + (uint64_t)i * 16u, v);
  else if (code == 1u)   // pairs: first row << 4 | second row; a last single row: bytes 0-7 | bytes 8-15 << 4
  {
    if (i & 1u) return;
    if (i + 1u < cnt) st128(body + (uint64_t)i * 8u, (v << 4) | rm_ld_row(a.ranks, s.row + 1u));
    else st64(body + (uint64_t)i * 8u, ((uint64_t)v[0] | (uint64_t)v[1] << 32) | ((uint64_t)v[2] | (uint64_t)v[3] << 32) << 4);
  }
  else if (code == 3u)   // groups of 4 rows in 16 bytes; the rest a dword each, the row's four dwords at 2 bit steps
  {
    const uint32_t full = cnt & ~3u;
    if (i < full)
    {
      if (i & 3u) return;
      st128(body + (uint64_t)i * 4u, v | rm_ld_row(a.ranks, s.row + 1u) << 2 | rm_ld_row(a.ranks, s.row + 2u) << 4 | rm_ld_row(a.ranks, s.row + 3u) << 6);
    }
    else st32(body + (uint64_t)i * 4u, v[0] | v[1] << 2 | v[2] << 4 | v[3] << 6);
  }
  else                   // groups of 6 rows in 36 bytes: rows 0 1 and the low 2 bits of row 2, the same of rows 3 4 5, bit 2 of rows 2 and 5
  {
    const uint32_t full = cnt / 6u * 6u;
    if (i < full)
    {
      if (i % 6u) return;
      const u32x4 p1 = rm_ld_row(a.ranks, s.row + 1u), p2 = rm_ld_row(a.ranks, s.row + 2u), p3 = rm_ld_row(a.ranks, s.row + 3u);
      const u32x4 p4 = rm_ld_row(a.ranks, s.row + 4u), p5 = rm_ld_row(a.ranks, s.row + 5u);
      uint8_t *g = body + (uint64_t)i * 6u;
      st128(g, v | p1 << 3 | (p2 & 0x03030303u) << 6);
      st128(g + 16, p3 | p4 << 3 | (p5 & 0x03030303u) << 6);
      st32(g + 32, rm_movemask(p2, 2u) | rm_movemask(p5, 2u) << 16);
    }
    else
    {
      uint8_t *g = body + (uint64_t)i * 6u;
      st16(g, rm_movemask(v, 0u));
      st16(g + 2, rm_movemask(v, 1u));
      st16(g + 4, rm_movemask(v, 2u));
    }
  }
}

template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_rm_emit(RmEncArgs a)
{
  const uint32_t lane = threadIdx.x & 63u, span = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (span >= a.spans || a.ctrl[0] != 0u) return;
  d_rm_emit(a, span, lane);
}

// ------------------------------------------------------------------------------------------------------------------
// decode

struct RmDecArgs
{
  const uint8_t *stream;
  uint8_t *ranks;        // 16-byte aligned
  uint4 *rec;            // x = body offset, y = first row, z = count, w = width code (COPY) or 4 | rank << 8 (RLE)
  uint32_t *ctrl;        // [0] status, [1] records, [2] offset of the tail ranks
  uint32_t *status;
  uint32_t streamCap, size, rows, maxRec;
};

// 16 bytes of the stream at `at`, zeros from `S` on
__device__ __forceinline__ u32x4 rm_ld_stream(const uint8_t *stream, uint64_t at, uint32_t S)
{
  u32x4 v = { 0u, 0u, 0u, 0u };
  if (at + 16u <= S) return ld128(stream + at);
  for (uint32_t k = 0; k < 16u && at + k < S; k++) v[k >> 2] |= (uint32_t)stream[at + k] << (8u * (k & 3u));
  return v;
}

constexpr uint32_t kRmWalkWindow = 1024u;

// One wave that is a workgroup of its own (the window's refill is a barrier); sWin: kRmWalkWindow bytes of LDS, 16-byte aligned.  Reads nothing of the
// stream at or behind a.streamCap; writes the records, a.ctrl[0 .. 2] and *a.status.
__device__ __forceinline__ void d_rm_walk(const RmDecArgs &a, uint8_t *sWin, uint32_t lane)
{
  constexpr uint32_t kWin = kRmWalkWindow, kStep = kWin - 16u, kNeed = 8u;   // a header is at most 5 bytes
  const uint32_t R = a.rows;
  uint32_t status = kRmDone, n = 0u, row = 0u;
  uint64_t pos = 8u;
  uint32_t S = 0u;
  if (a.streamCap < 10u) status = kRmMalformed;
  else
  {
    S = ld32(a.stream + 4);
    if (ld32(a.stream) != a.size || S > a.streamCap || S < 10u) status = kRmMalformed;
  }
  uint64_t win = 0u;
  u32x4 next = { 0u, 0u, 0u, 0u };
  bool have = false;
  // the window holds [win, win + kWin); after this call it holds [pos, pos + kNeed)
  auto ensure = [&]() {
    if (have && pos >= win && pos + kNeed <= win + kWin) return;
    __syncthreads();
    if (have && pos >= win + kStep && pos + kNeed <= win + kStep + kWin) win += kStep;   // the window that was asked for ahead
    else { win = pos; next = rm_ld_stream(a.stream, win + lane * 16u, S); }
    lds_st128(sWin + lane * 16u, next);
    next = rm_ld_stream(a.stream, win + kStep + lane * 16u, S);
    have = true;
    __syncthreads();
  };
  auto byte_at = [&](uint32_t k) -> uint32_t { return sWin[(uint32_t)(pos - win) + k]; };
  auto word_at = [&]() -> uint32_t { return byte_at(0) | byte_at(1) << 8 | byte_at(2) << 16 | byte_at(3) << 24; };
  while (status == kRmDone)
  {
    // COPY
    ensure();
    uint32_t b = byte_at(0), h = (b & 1u) ? 4u : 1u;
    if (pos + h > S) { status = kRmMalformed; break; }
    uint32_t c = (b & 1u) ? word_at() >> 3 : b >> 3;
    const uint32_t code = (b >> 1) & 3u;
    const uint64_t body = (uint64_t)c * rm_row_bytes(code);
    if (c > R - row || pos + h + body > S || (c != 0u && n >= a.maxRec)) { status = kRmMalformed; break; }
    if (c != 0u)
    {
      if (lane == 0u) a.rec[n] = make_uint4((uint32_t)(pos + h), row, c, code);
      n++;
    }
    row += c;
    pos += h + body;
    // RLE
    ensure();
    b = byte_at(0);
    h = (b & 1u) ? 4u : 1u;
    if (pos + h > S) { status = kRmMalformed; break; }
    c = (b & 1u) ? word_at() >> 1 : b >> 1;
    if (c == 0u) { pos += h; break; }
    if (c > R - row || pos + h + 1u > S || n >= a.maxRec) { status = kRmMalformed; break; }
    if (lane == 0u) a.rec[n] = make_uint4((uint32_t)(pos + h), row, c, 4u | byte_at(h) << 8);
    n++;
    row += c;
    pos += h + 1u;
  }
  if (status == kRmDone && (row != R || pos + (a.size - R * 16u) > S)) status = kRmMalformed;
  if (lane == 0u)
  {
    a.ctrl[0] = status;
    a.ctrl[1] = n;
    a.ctrl[2] = (uint32_t)pos;
    *a.status = status;
  }
}

template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_rm_walk(RmDecArgs a)
{
  __shared__ __attribute__((aligned(16))) uint8_t sWin[kRmWalkWindow];
  d_rm_walk(a, sWin, threadIdx.x);
}

// a wave: rows row0 .. row0 + 63 (row0 < a.rows) into the rank buffer
__device__ __forceinline__ void d_rm_expand(const RmDecArgs &a, uint32_t row0, uint32_t lane)
{
  const uint32_t R = a.rows;
  const uint32_t n = a.ctrl[1];
  // the packet of the span's first row (the records cover rows 0 .. R without a gap, record 0 starts at row 0) ...
  uint32_t lo = 0u, hi = n;
  while (hi - lo > 1u)
  {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (a.rec[mid].y <= row0) lo = mid; else hi = mid;
  }
  const uint32_t row = row0 + lane;
  if (row >= R) return;
  // ... and the lane's own among the next 64
  hi = umin(n, lo + 64u);
  while (hi - lo > 1u)
  {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (a.rec[mid].y <= row) lo = mid; else hi = mid;
  }
  const uint4 q = a.rec[lo];
  const uint32_t i = row - q.y, c = q.z, code = q.w & 0xFFu;
  const uint8_t *p = a.stream + q.x;
  u32x4 v;
  if (code == 4u)
  {
    const uint32_t s = (q.w >> 8) * 0x01010101u;
    v[0] = s; v[1] = s; v[2] = s; v[3] = s;
  }
  else if (code == 0u)
    v = ld128(p + (uint64_t)i * 16u);
  else if (code == 1u)
  {
    if (i < (c & ~1u))
    {
      const u32x4 g = ld128(p + (uint64_t)(i >> 1) * 16u);
      v = ((i & 1u) ? g : g >> 4) & 0x0F0F0F0Fu;
    }
    else
    {
      const uint64_t g = ld64(p + (uint64_t)i * 8u), l = g & 0x0F0F0F0F0F0F0F0Full, u = (g >> 4) & 0x0F0F0F0F0F0F0F0Full;
      v[0] = (uint32_t)l; v[1] = (uint32_t)(l >> 32); v[2] = (uint32_t)u; v[3] = (uint32_t)(u >> 32);
    }
  }
  else if (code == 3u)
  {
    if (i < (c & ~3u))
      v = (ld128(p + (uint64_t)(i >> 2) * 16u) >> (2u * (i & 3u))) & 0x03030303u;
    else
    {
      const uint32_t g = ld32(p + (uint64_t)i * 4u);
      v[0] = g & 0x03030303u; v[1] = (g >> 2) & 0x03030303u; v[2] = (g >> 4) & 0x03030303u; v[3] = (g >> 6) & 0x03030303u;
    }
  }
  else
  {
    const uint32_t full = c / 6u * 6u;
    if (i < full)
    {
      const uint32_t j = i % 6u, jj = j % 3u;
      const uint8_t *g = p + (uint64_t)(i / 6u) * 36u;
      const u32x4 w = ld128(g + (j >= 3u ? 16u : 0u));
      if (jj == 0u) v = w & 0x07070707u;
      else if (jj == 1u) v = (w >> 3) & 0x07070707u;
      else v = ((w >> 6) & 0x03030303u) | rm_spread(ld16(g + 32u + (j == 5u ? 2u : 0u))) << 2;
    }
    else
    {
      const uint8_t *g = p + (uint64_t)i * 6u;
      v = rm_spread(ld16(g)) | rm_spread(ld16(g + 2)) << 1 | rm_spread(ld16(g + 4)) << 2;
    }
  }
  *(u32x4 *)__builtin_assume_aligned(a.ranks + (uint64_t)row * 16u, 16) = v;
}
// the tail ranks behind the rows: lanes 0 .. 14
__device__ __forceinline__ void d_rm_expand_tail(const RmDecArgs &a, uint32_t lane)
{
  const uint32_t R = a.rows;
  if (lane < a.size - R * 16u) a.ranks[(uint64_t)R * 16u + lane] = a.stream[a.ctrl[2] + lane];
}

template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_rm_expand(RmDecArgs a)
{
  if (a.ctrl[0] != kRmDone) return;
  const uint32_t lane = threadIdx.x & 63u, row0 = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;
  if (blockIdx.x == 0u) d_rm_expand_tail(a, threadIdx.x);
  if (row0 >= a.rows) return;
  d_rm_expand(a, row0, lane);
}

}   // namespace hsrle
