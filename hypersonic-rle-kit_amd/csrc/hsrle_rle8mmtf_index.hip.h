// hsrle_rle8mmtf_index.hip.h -- the ENTRY INDEX of an rle8_mmtf128 stream (hsrle_rle8mmtf.hip.h has the stream): a sidecar that names packet headers of
// the chain, so that the chain -- the format's one serial dependence -- is followed by a wave per stretch between two entries instead of one wave.
//
// Index: 64 header bytes (magic "HSRLEMFI", u32 version 1, u32 headerBytes 64, u32 uncompressedSize, u32 streamSize, u32 spacingRows, u32 entryCount,
// u64 indexSize = 64 + 16 entryCount, zeros), then the entries: u32 offset (of the packet's own header byte), u32 row (its first row), u32 ordinal (the
// non-null packets in front of it = its record in the list d_rm_expand searches), u32 kind (0 COPY, 1 RLE).  THE RULE, with R rows and windows of
// `spacing` rows: for every j >= 1 with j spacing < R the first non-null packet whose first row lies in window j, if there is one, in order of j.  The
// chain's start (offset 8, row 0, ordinal 0, COPY) is not stored.
//
// Decode with an index:
//   k_rm_index_begin    one wave: the stream header against the arguments (MALFORMED), the index header against the caller's (INDEX); INITIALISES ctrl[0]
//   k_rm_walk_indexed   a wave per stretch: d_rm_walk started at an entry, records from rec[ordinal] on, up to the next entry, where it has to stand on
//                       exactly that entry's offset, row, ordinal and kind.  The index is trusted in nothing: every wave checks its two entries first, and
//                       a wave's records stay inside [its ordinal, the next entry's ordinal).  By induction over the stretches (stretch 0 starts at the
//                       chain's true start, every stretch ends in the state the next one starts from) an index that passes gives the serial walk's record
//                       list.  Any failure is an OR of INDEX into ctrl[0]; the last stretch does the serial walk's end-of-chain checks
//   k_rm_expand_indexed k_rm_expand, gated on ctrl[0] as it is; also hands ctrl[0] to the caller's status word
// Index of a foreign stream:
//   k_rm_index_build    ONE wave, the serial walk without records: emits the entries by the rule; header and size word only behind a good chain
// Index from the encoder (behind k_rm_emit, from what classify and scan left per span; any span length gives the same index):
//   k_rm_index_count    one workgroup: per span the packet starts and the entries in front of it (into res[].y / .z, which k_rm_emit is done with); header
//   k_rm_index_emit     a wave per span that holds an entry: a start is an entry if no start lies between its window's first row and itself
#pragma once

#include "hsrle_rle8mmtf.hip.h"

namespace hsrle {

constexpr uint32_t kRmIndex = 3u;            // == HSRLE_RLE8_MMTF_INDEX (include/hsrle.h)
constexpr uint32_t kRmIndexHeader = 64u, kRmIndexEntry = 16u;

struct RmIndexHeader { uint32_t w[16]; };   // the 64 header bytes as words

// word i of the header (a chain of selects: an array indexed by the lane would be an alloca per lane)
__host__ __device__ __forceinline__ uint32_t rm_index_header_word(uint32_t i, uint32_t size, uint32_t streamSize, uint32_t spacing, uint32_t entries)
{
  const uint64_t bytes = kRmIndexHeader + (uint64_t)kRmIndexEntry * entries;
  switch (i)
  {
  case 0: return 0x4C525348u;   // "HSRL"
  case 1: return 0x49464D45u;   // "EMFI"
  case 2: return 1u;
  case 3: return kRmIndexHeader;
  case 4: return size;
  case 5: return streamSize;
  case 6: return spacing;
  case 7: return entries;
  case 8: return (uint32_t)bytes;
  case 9: return (uint32_t)(bytes >> 32);
  default: return 0u;
  }
}

struct RmEntry { uint32_t offset, row, ordinal, kind; };
__device__ __forceinline__ RmEntry rm_ld_entry(const uint8_t *index, uint32_t k)
{
  const u32x4 v = ld128(index + kRmIndexHeader + (uint64_t)kRmIndexEntry * k);
  return { v[0], v[1], v[2], v[3] };
}
__device__ __forceinline__ void rm_st_entry(uint8_t *index, uint32_t k, uint32_t offset, uint32_t row, uint32_t ordinal, uint32_t kind)
{
  const u32x4 v = { offset, row, ordinal, kind };
  st128(index + kRmIndexHeader + (uint64_t)kRmIndexEntry * k, v);
}

struct RmIdxDecArgs
{
  RmDecArgs d;             // d.ctrl: [0] status, [1] records, [2] offset of the tail ranks, [3] the stream header's streamSize
  const uint8_t *index;
  RmIndexHeader want;      // the index header the caller holds
  uint32_t entries;
};

// The chain from (pos, row, n), beginning with its RLE half if `rle`; S: the stream's size.  Returns false where d_rm_walk says malformed.
//   RECORDS: a record per non-null packet, as d_rm_walk writes them; with hasEnd (end: the next entry) the walk stops when it stands on end.offset and is
//            good only if it stands there in exactly the entry's state; it never writes rec[end.ordinal] or behind, never passes end.offset or end.row.
//   else:    no records; an entry per window by the rule into `index`, *emitted counts them.
// Without hasEnd the chain has to end as d_rm_walk wants it; pos is then the offset of the tail ranks.
template <bool RECORDS>
__device__ __forceinline__ bool d_rm_walk_from(const RmDecArgs &a, uint8_t *sWin, uint32_t lane, uint32_t S, uint64_t &pos, uint32_t &row, uint32_t &n, bool rle, bool hasEnd, RmEntry end,
                                               uint8_t *index, uint32_t spacing, uint32_t *emitted)
{
  constexpr uint32_t kWin = kRmWalkWindow, kStep = kWin - 16u, kNeed = 8u;
  const uint32_t R = a.rows;
  const uint32_t rowEnd = hasEnd ? end.row : R, recEnd = hasEnd ? end.ordinal : a.maxRec;
  uint64_t win = 0u;
  u32x4 next = { 0u, 0u, 0u, 0u };
  bool have = false;
  uint32_t lastWindow = 0u, e = 0u;
  auto ensure = [&]() {
    if (have && pos >= win && pos + kNeed <= win + kWin) return;
    __syncthreads();
    if (have && pos >= win + kStep && pos + kNeed <= win + kStep + kWin) win += kStep;
    else { win = pos; next = rm_ld_stream(a.stream, win + lane * 16u, S); }
    lds_st128(sWin + lane * 16u, next);
    next = rm_ld_stream(a.stream, win + kStep + lane * 16u, S);
    have = true;
    __syncthreads();
  };
  auto byte_at = [&](uint32_t k) -> uint32_t { return sWin[(uint32_t)(pos - win) + k]; };
  auto word_at = [&]() -> uint32_t { return byte_at(0) | byte_at(1) << 8 | byte_at(2) << 16 | byte_at(3) << 24; };
  // 1: the walk stands on `end`, in its state or not (good says which); 2: it has passed it
  auto landing = [&](uint32_t kind, bool &good) -> uint32_t {
    if (!hasEnd) return 0u;
    if (pos == end.offset) { good = row == end.row && n == end.ordinal && kind == end.kind; return 1u; }
    return (pos > end.offset || row > end.row) ? 2u : 0u;
  };
  auto packet = [&](uint32_t at, uint32_t c, uint32_t kind, uint32_t w) {
    if (RECORDS) { if (lane == 0u) a.rec[n] = make_uint4(at, row, c, w); }
    else
    {
      const uint32_t j = row / spacing;
      if (j > lastWindow)
      {
        if (lane == 0u) rm_st_entry(index, e, (uint32_t)pos, row, n, kind);
        lastWindow = j;
        e++;
      }
    }
    n++;
  };
  bool ok = false, good = false;
  for (;;)
  {
    if (!rle)
    {
      if (const uint32_t l = landing(0u, good)) { ok = l == 1u && good; break; }
      ensure();
      const uint32_t b = byte_at(0), h = (b & 1u) ? 4u : 1u;
      if (pos + h > S) break;
      const uint32_t c = (b & 1u) ? word_at() >> 3 : b >> 3, code = (b >> 1) & 3u;
      const uint64_t body = (uint64_t)c * rm_row_bytes(code);
      if (c > rowEnd - row || pos + h + body > S || (c != 0u && n >= recEnd)) break;
      if (c != 0u) packet((uint32_t)(pos + h), c, 0u, code);
      row += c;
      pos += h + body;
    }
    rle = false;
    if (const uint32_t l = landing(1u, good)) { ok = l == 1u && good; break; }
    ensure();
    const uint32_t b = byte_at(0), h = (b & 1u) ? 4u : 1u;
    if (pos + h > S) break;
    const uint32_t c = (b & 1u) ? word_at() >> 1 : b >> 1;
    if (c == 0u)
    {
      pos += h;
      ok = !hasEnd && row == R && pos + (a.size - R * 16u) <= S;   // (a chain that ends in front of the next entry has missed it)
      break;
    }
    if (c > rowEnd - row || pos + h + 1u > S || n >= recEnd) break;
    packet((uint32_t)(pos + h), c, 1u, 4u | byte_at(h) << 8);
    row += c;
    pos += h + 1u;
  }
  if (!RECORDS) *emitted = e;
  return ok;
}

// the stream header against the arguments, as d_rm_walk reads it: the stream's size, 0 = malformed
__device__ __forceinline__ uint32_t rm_stream_size(const RmDecArgs &a)
{
  if (a.streamCap < 10u) return 0u;
  const uint32_t S = ld32(a.stream + 4);
  return (ld32(a.stream) != a.size || S > a.streamCap || S < 10u) ? 0u : S;
}

template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_rm_index_begin(RmIdxDecArgs a)
{
  const uint32_t lane = threadIdx.x;
  const uint32_t S = rm_stream_size(a.d);
  const bool differs = lane < 16u && ld32(a.index + lane * 4u) != a.want.w[lane];
  const bool stale = __ballot(differs) != 0ull || a.want.w[5] != S;
  if (lane == 0u)
  {
    a.d.ctrl[0] = S == 0u ? kRmMalformed : (stale ? kRmIndex : kRmDone);
    a.d.ctrl[1] = 0u;
    a.d.ctrl[2] = 0u;
    a.d.ctrl[3] = S;
  }
}

// an entry's own bounds; its order behind the entry in front of it
__device__ __forceinline__ bool rm_entry_in_bounds(const RmEntry &e, uint32_t S, uint32_t R, uint32_t maxRec)
{
  return e.offset >= 8u && e.offset < S && e.row < R && e.ordinal < maxRec && e.ordinal <= e.row && e.kind <= 1u;
}
__device__ __forceinline__ bool rm_entry_behind(const RmEntry &e, const RmEntry &prev) { return e.offset > prev.offset && e.row > prev.row && e.ordinal > prev.ordinal; }

// One wave that is a workgroup of its own, as k_rm_walk is: stretch blockIdx.x of a.entries + 1.
template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_rm_walk_indexed(RmIdxDecArgs a)
{
  __shared__ __attribute__((aligned(16))) uint8_t sWin[kRmWalkWindow];
  if (a.d.ctrl[0] != kRmDone) return;
  const uint32_t lane = threadIdx.x, k = blockIdx.x, S = a.d.ctrl[3], R = a.d.rows;
  const RmEntry origin = { 8u, 0u, 0u, 0u };
  const bool last = k == a.entries;
  RmEntry from = origin, to = origin;
  bool ok = true;
  if (k != 0u)
  {
    from = rm_ld_entry(a.index, k - 1u);
    ok = rm_entry_in_bounds(from, S, R, a.d.maxRec);   // (its order behind the entry in front of it: the stretch in front)
  }
  if (!last)
  {
    to = rm_ld_entry(a.index, k);
    ok = ok && rm_entry_in_bounds(to, S, R, a.d.maxRec) && rm_entry_behind(to, from);
  }
  uint64_t pos = from.offset;
  uint32_t row = from.row, n = from.ordinal;
  if (ok) ok = d_rm_walk_from<true>(a.d, sWin, lane, S, pos, row, n, from.kind == 1u, !last, to, nullptr, 0u, nullptr);
  if (lane != 0u) return;
  if (!ok) atomicOr(&a.d.ctrl[0], kRmIndex);
  else if (last)
  {
    a.d.ctrl[1] = n;
    a.d.ctrl[2] = (uint32_t)pos;
  }
}

template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_rm_expand_indexed(RmDecArgs a)
{
  const uint32_t status = a.ctrl[0];
  if (blockIdx.x == 0u && threadIdx.x == 0u) *a.status = status;
  if (status != kRmDone) return;
  const uint32_t lane = threadIdx.x & 63u, row0 = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;
  if (blockIdx.x == 0u) d_rm_expand_tail(a, threadIdx.x);
  if (row0 >= a.rows) return;
  d_rm_expand(a, row0, lane);
}

struct RmIdxBuildArgs
{
  RmDecArgs d;             // stream, streamCap, size, rows, status; no records, no rank buffer, no control words
  uint8_t *index;
  uint64_t *indexSize;
  uint32_t spacing;
};

template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_rm_index_build(RmIdxBuildArgs a)
{
  __shared__ __attribute__((aligned(16))) uint8_t sWin[kRmWalkWindow];
  const uint32_t lane = threadIdx.x, S = rm_stream_size(a.d);
  uint64_t pos = 8u;
  uint32_t row = 0u, n = 0u, entries = 0u;
  const bool ok = S != 0u && d_rm_walk_from<false>(a.d, sWin, lane, S, pos, row, n, false, false, RmEntry{ 0u, 0u, 0u, 0u }, a.index, a.spacing, &entries);
  if (ok && lane < 16u) st32(a.index + lane * 4u, rm_index_header_word(lane, a.d.size, S, a.spacing, entries));
  if (lane == 0u)
  {
    *a.indexSize = ok ? kRmIndexHeader + (uint64_t)kRmIndexEntry * entries : 0ull;
    *a.d.status = ok ? kRmDone : kRmMalformed;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// from the encoder, behind k_rm_emit

struct RmIdxEncArgs
{
  RmEncArgs e;             // e.outSize: the stream's size as k_rm_scan left it; e.ctrl[0] = 1: the stream did not fit
  uint8_t *index;
  uint64_t *indexSize;
  uint32_t spacing;
};

// row of the last packet start in front of `span`, kRmNone if there is none (span 0)
__device__ __forceinline__ uint32_t rm_start_in_front(const RmEncArgs &a, uint32_t span)
{
  const uint32_t p = a.res[span].w;
  return (span == 0u || p == kRmNone) ? kRmNone : p * a.SP + ((a.sum[p].x >> 16) & 0xFFu);
}
// A span is at most 64 rows and a window at least 64, so a span's starts lie in at most two windows.  Its entries: its first start, if no start lies
// between that start's window edge and it (and the window is not window 0); its first start in the next window, if it has one there.
__device__ __forceinline__ uint32_t rm_span_entries(const RmEncArgs &a, uint32_t span, uint32_t spacing, uint4 q)
{
  if ((q.x & 0xFFu) == 0u) return 0u;
  const uint32_t first = span * a.SP + ((q.x >> 8) & 0xFFu), last = span * a.SP + ((q.x >> 16) & 0xFFu), j = first / spacing;
  const uint32_t front = rm_start_in_front(a, span);
  const uint32_t own = (j != 0u && (front == kRmNone || front < j * spacing)) ? 1u : 0u;
  return own + (last / spacing > j ? 1u : 0u);
}

// One workgroup of T threads, a run of spans per thread (sA, sB: T words of LDS each).  res[].y = packet starts in front of the span,
// res[].z = entries in front of it | its own entries << 28.  Returns the number of entries.
template <uint32_t T>
__device__ __forceinline__ uint32_t d_rm_index_count(const RmEncArgs &a, uint32_t spacing, uint32_t t, uint32_t *sA, uint32_t *sB, uint32_t *sTotal)
{
  const uint32_t N = a.spans;
  const uint32_t per = (N + T - 1u) / T;
  const uint64_t lo64 = (uint64_t)t * per;
  const uint32_t lo = (uint32_t)(lo64 < N ? lo64 : N), hi = (uint32_t)(lo64 + per < N ? lo64 + per : N);
  uint32_t starts = 0u, entries = 0u;
  for (uint32_t k = lo; k < hi; k++)
  {
    const uint4 q = a.sum[k];
    starts += q.x & 0xFFu;
    entries += rm_span_entries(a, k, spacing, q);
  }
  sA[t] = starts;
  sB[t] = entries;
  __syncthreads();
  if (t == 0u)
  {
    uint32_t s = 0u, e = 0u;
    for (uint32_t i = 0; i < T; i++)
    {
      const uint32_t x = sA[i], y = sB[i];
      sA[i] = s;
      sB[i] = e;
      s += x;
      e += y;
    }
    *sTotal = e;
  }
  __syncthreads();
  starts = sA[t];
  entries = sB[t];
  for (uint32_t k = lo; k < hi; k++)
  {
    const uint4 q = a.sum[k];
    const uint32_t own = rm_span_entries(a, k, spacing, q);
    uint4 r = a.res[k];
    r.y = starts;
    r.z = entries | own << 28;
    a.res[k] = r;
    starts += q.x & 0xFFu;
    entries += own;
  }
  return *sTotal;
}

template <int UNUSED = 0>
__global__ __launch_bounds__(1024) void k_rm_index_count(RmIdxEncArgs a)
{
  __shared__ uint32_t sA[kRmScanThreads], sB[kRmScanThreads];
  __shared__ uint32_t sTotal;
  const uint32_t entries = d_rm_index_count<kRmScanThreads>(a.e, a.spacing, threadIdx.x, sA, sB, &sTotal);
  const bool fits = a.e.ctrl[0] == 0u;
  if (fits && threadIdx.x < 16u) st32(a.index + threadIdx.x * 4u, rm_index_header_word(threadIdx.x, a.e.size, *a.e.outSize, a.spacing, entries));
  if (threadIdx.x == 0u) *a.indexSize = fits ? kRmIndexHeader + (uint64_t)kRmIndexEntry * entries : 0ull;
}

// a wave: the entries of one span
__device__ __forceinline__ void d_rm_index_emit(const RmIdxEncArgs &a, uint32_t span, uint32_t lane)
{
  const uint4 r = a.e.res[span];
  if ((r.z >> 28) == 0u) return;
  RmSpan s;
  rm_span_load(a.e.ranks, a.e.rows, a.e.SP, span, lane, s);
  const uint32_t last = 63u - (uint32_t)__builtin_clzll(s.M);   // (a span with an entry has a start)
  // the stream offset of every start: only the packets that begin AND end in the span lie in front of another start of it
  const uint32_t bytes = (s.start && lane != last) ? s.pre + rm_packet_bytes(s.rle, s.segEnd - lane, rm_width_code(s.orSeg)) : 0u;
  uint32_t inc = bytes;
#pragma unroll
  for (uint32_t o = 1; o < 64u; o <<= 1)
  {
    const uint32_t y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  const uint64_t below = s.M & ((1ull << lane) - 1ull);
  const uint32_t front = below ? span * a.e.SP + 63u - (uint32_t)__builtin_clzll(below) : rm_start_in_front(a.e, span);
  const uint32_t j = s.row / a.spacing;
  const bool entry = s.start && j != 0u && (front == kRmNone || front < j * a.spacing);
  const uint64_t E = __ballot(entry);
  if (entry)
    rm_st_entry(a.index, (r.z & 0x0FFFFFFFu) + (uint32_t)__popcll(E & ((1ull << lane) - 1ull)), r.x + inc - bytes + s.pre, s.row, r.y + (uint32_t)__popcll(below), s.rle ? 1u : 0u);
}

template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_rm_index_emit(RmIdxEncArgs a)
{
  const uint32_t lane = threadIdx.x & 63u, span = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (span >= a.e.spans || a.e.ctrl[0] != 0u) return;
  d_rm_index_emit(a, span, lane);
}

}   // namespace hsrle
