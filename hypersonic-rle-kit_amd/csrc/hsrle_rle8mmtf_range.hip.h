// hsrle_rle8mmtf_range.hip.h -- BYTE-RANGE DECODE of an rle8_mmtf128 stream (hsrle_rle8mmtf.hip.h has the stream, hsrle_rle8mmtf_index.hip.h its entry index):
// the index lets the header chain be entered in the middle; the CHECKPOINTS, a second sidecar, do the same for the sixteen move-to-front lists.
//
// Checkpoints: 64 header bytes (magic "HSRLEMFC", u32 version 1, u32 headerBytes 64, u32 uncompressedSize, u32 streamSize, u32 checkpointRows,
// u32 checkpointCount, u64 size = 64 + 4096 checkpointCount, zeros), then per k = 1 .. checkpointCount the sixteen lists in front of row k checkpointRows:
// column c's at bytes [256 c, 256 c + 256), byte i the symbol of rank i (a plain layout, not the state table's).  checkpointCount = (R - 1) / checkpointRows.
//
// Build (behind the indexed decode's walk and expansion and passes A and B of the mmtf128 decode plan, which leave the list in front of every segment):
//   k_rm_checkpoint_lists  a lane per (checkpoint, column): the list of the segment that holds the checkpoint's row, the ranks from the segment's first row to
//                          that row applied to it, stored plain; header and size word behind a DONE verdict only
// Range decode of output bytes [offset, offset + length): r0 = offset / 16 (at most R - 1), r1 = ceil((offset + length) / 16) (at most R),
// c = the last checkpoint row <= r0:
//   k_rm_range_begin   one wave: the stream header against the arguments (MALFORMED), the two sidecars' headers against the caller's (INDEX, CHECKPOINT), every
//                      list of the checkpoint of row c a permutation of 0 .. 255 (CHECKPOINT), e0 = the last entry with row <= c; INITIALISES the control words
//   k_rm_walk_range    wave i: the stretch of entry e0 + i, with k_rm_walk_indexed's entry checks and landing rule; it exits where the stretch begins at or
//                      behind row r1.  Records relative to e0's ordinal, bounded by the record table's capacity
//   k_rm_expand_range  the last verdict (the stretches that ran are e0 .. the one that reaches r1, without a gap), the caller's status word; rank rows [c, r1)
//                      into the rank buffer at row - c, the tail ranks if r1 = R
//   pass A of the mmtf128 decode plan of r1 - c rows as it is (a segment's permutation does not depend on the list it is applied to),
//   k_rm_range_scan    pass B with the checkpoint's column list in front of segment 0,
//   k_rm_range_rows    pass C with segment 0 run from the checkpoint, into a staging area of the workspace
//   k_rm_range_copy    behind a DONE verdict: staging[offset - 16 c, + length) to the caller's buffer, the only kernel that has its address
// Neither sidecar is trusted for memory safety: entries and packets are bounds-checked as in the indexed decode, the records a stretch may write are bounded
// before it walks, and a rank only ever indexes a 256-entry list, whatever the checkpoint holds.
#pragma once

#include "hsrle_mmtf.hip.h"
#include "hsrle_rle8mmtf_index.hip.h"

namespace hsrle {

constexpr uint32_t kRmCheckpoint = 4u;       // == HSRLE_RLE8_MMTF_CHECKPOINT (include/hsrle.h)
constexpr uint32_t kRmCkptHeader = 64u, kRmCkptBytes = 4096u;

__host__ __device__ __forceinline__ uint32_t rm_ckpt_header_word(uint32_t i, uint32_t size, uint32_t streamSize, uint32_t checkpointRows, uint32_t count)
{
  const uint64_t bytes = kRmCkptHeader + (uint64_t)kRmCkptBytes * count;
  switch (i)
  {
  case 0: return 0x4C525348u;   // "HSRL"
  case 1: return 0x43464D45u;   // "EMFC"
  case 2: return 1u;
  case 3: return kRmCkptHeader;
  case 4: return size;
  case 5: return streamSize;
  case 6: return checkpointRows;
  case 7: return count;
  case 8: return (uint32_t)bytes;
  case 9: return (uint32_t)(bytes >> 32);
  default: return 0u;
  }
}

// the lane's list from 256 plain bytes at any address, and back
__device__ __forceinline__ void rm_list_load_plain(MmtfList &L, const uint8_t *p)
{
  L.head = ld32(p);
  for (uint32_t j = 1; j < 64u; j++) L.lds[j * 64u] = ld32(p + 4u * j);
}
__device__ __forceinline__ void rm_list_store_plain(const MmtfList &L, uint8_t *p)
{
  st32(p, L.head);
  for (uint32_t j = 1; j < 64u; j++) st32(p + 4u * j, L.lds[j * 64u]);
}
// the lane's dword 0 of (segment, column) in the state table of the mmtf128 plan
__device__ __forceinline__ uint32_t *rm_table_slot(uint32_t *table, uint32_t seg, uint32_t col)
{
  const uint32_t id = seg * 16u + col;
  return table + (uint64_t)(id >> 6) * kMmtfGroupDwords + (id & 63u);
}

// ------------------------------------------------------------------------------------------------------------------
// build

struct RmCkptArgs
{
  const uint8_t *ranks;    // the whole stream's rank buffer
  uint32_t *table;         // the state table behind pass B: slot s = the list in front of segment s (not written for one segment)
  const uint32_t *ctrl;    // [0] the indexed walk's verdict, [3] the stream's size
  uint8_t *out;
  uint64_t *outSize;
  uint32_t size, segRows, checkpointRows, count;
};

// One wave per 4 checkpoints: lane = (checkpoint, column), as a wave of pass A is (segment, column).
template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_rm_checkpoint_lists(RmCkptArgs a)
{
  __shared__ uint32_t sList[kMmtfGroupDwords];
  __shared__ __attribute__((aligned(16))) uint8_t sTile[1024];
  const uint32_t lane = threadIdx.x, status = a.ctrl[0];
  if (blockIdx.x == 0u)
  {
    if (status == kRmDone && lane < 16u) st32(a.out + lane * 4u, rm_ckpt_header_word(lane, a.size, a.ctrl[3], a.checkpointRows, a.count));
    if (lane == 0u) *a.outSize = status == kRmDone ? kRmCkptHeader + (uint64_t)kRmCkptBytes * a.count : 0ull;
  }
  if (status != kRmDone) return;
  const uint32_t k = blockIdx.x * 4u + lane / 16u + 1u, col = lane % 16u;
  const bool valid = k <= a.count;
  const uint32_t row = valid ? k * a.checkpointRows : 0u, seg = row / a.segRows, first = seg * a.segRows;
  MmtfList L;
  L.lds = sList + lane;
  if (seg != 0u) L.load(rm_table_slot(a.table, seg, col)); else L.identity();
  uint32_t K = 0u;
  d_mmtf_rows<16, true, false>(L, K, a.ranks + (uint64_t)first * 16u, nullptr, row - first, (a.segRows + 15u) / 16u, col, sTile + (lane / 16u) * 256u);
  if (valid) rm_list_store_plain(L, a.out + kRmCkptHeader + (uint64_t)(k - 1u) * kRmCkptBytes + col * 256u);
}

// ------------------------------------------------------------------------------------------------------------------
// range decode

struct RmRangeArgs
{
  RmDecArgs d;             // d.ranks: the rank buffer, row c at 0; d.rec: record 0 is e0's ordinal; d.maxRec: the records the table holds; d.rows: R
                           // d.ctrl: [0] status, [1] records, [2] offset of the tail ranks, [3] the stream's size, [4] e0's stretch (0: the chain's start),
                           //         [5] the last verdict, [6] the first wave that found nothing to do, [7] the last wave that walked,
                           //         [8] 1: a wave reached r1 and left [1]
  const uint8_t *index, *ckpt;
  RmIndexHeader wantIndex, wantCkpt;   // the two headers the caller holds
  uint32_t entries;
  uint32_t c, r1;          // rows [c, r1) are expanded; c is 0 or a checkpoint's row
  const uint8_t *start;    // the checkpoint of row c, nullptr for c = 0
};

template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_rm_range_begin(RmRangeArgs a)
{
  __shared__ uint32_t sSeen[16][8];
  const uint32_t lane = threadIdx.x;
  const uint32_t S = rm_stream_size(a.d);
  const bool differsI = lane < 16u && ld32(a.index + lane * 4u) != a.wantIndex.w[lane];
  const bool differsC = lane < 16u && ld32(a.ckpt + lane * 4u) != a.wantCkpt.w[lane];
  const bool staleI = __ballot(differsI) != 0ull || a.wantIndex.w[5] != S;
  bool staleC = __ballot(differsC) != 0ull || a.wantCkpt.w[5] != S;
  if (a.start != nullptr)
  {
    // a 256-bit set per column: lane = (column, quarter of its list)
    for (uint32_t i = lane; i < 128u; i += 64u) sSeen[i >> 3][i & 7u] = 0u;
    __syncthreads();
    const uint32_t col = lane >> 2;
    const uint8_t *p = a.start + lane * 64u;
    for (uint32_t i = 0; i < 64u; i++)
    {
      const uint32_t x = p[i];
      atomicOr(&sSeen[col][x >> 5], 1u << (x & 31u));
    }
    __syncthreads();
    const bool hole = sSeen[lane >> 2][lane & 3u] != 0xFFFFFFFFu || sSeen[lane >> 2][4u + (lane & 3u)] != 0xFFFFFFFFu;
    staleC = staleC || __ballot(hole) != 0ull;
  }
  if (lane != 0u) return;
  // the last entry with row <= c, as a stretch number: 0 = the chain's start.  (Entries that are not in order make it any number of [0, entries]:
  // the stretch's wave checks what it starts from.)
  uint32_t lo = 0u, hi = a.entries;
  while (lo < hi)
  {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (rm_ld_entry(a.index, mid).row <= a.c) lo = mid + 1u; else hi = mid;
  }
  a.d.ctrl[0] = S == 0u ? kRmMalformed : (staleI ? kRmIndex : (staleC ? kRmCheckpoint : kRmDone));
  a.d.ctrl[1] = 0u;
  a.d.ctrl[2] = 0u;
  a.d.ctrl[3] = S;
  a.d.ctrl[4] = lo;
  a.d.ctrl[5] = kRmMalformed;
  a.d.ctrl[6] = 0xFFFFFFFFu;
  a.d.ctrl[7] = 0u;
  a.d.ctrl[8] = 0u;
}

// One wave that is a workgroup of its own: stretch ctrl[4] + blockIdx.x.
template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_rm_walk_range(RmRangeArgs a)
{
  __shared__ __attribute__((aligned(16))) uint8_t sWin[kRmWalkWindow];
  if (a.d.ctrl[0] != kRmDone) return;
  const uint32_t lane = threadIdx.x, i = blockIdx.x, S = a.d.ctrl[3], k0 = a.d.ctrl[4], R = a.d.rows, cap = a.d.maxRec;
  const uint32_t k = k0 + i;
  const RmEntry origin = { 8u, 0u, 0u, 0u };
  const RmEntry e0 = k0 != 0u ? rm_ld_entry(a.index, k0 - 1u) : origin;
  RmEntry from = e0, to = origin;
  if (i != 0u && k <= a.entries) from = rm_ld_entry(a.index, k - 1u);
  // nothing to do: no such stretch, or it begins at or behind r1 (a row that is only compared: the entry is not this range's to judge)
  if (k > a.entries || (i != 0u && from.row >= a.r1))
  {
    if (lane == 0u) atomicMin(&a.d.ctrl[6], i);
    return;
  }
  const bool last = k == a.entries;
  // e0 has nothing in front of it that vouches for it: its own bounds, and that row c lies in or behind its packet
  bool ok = (k0 == 0u || rm_entry_in_bounds(e0, S, R, R + 1u)) && e0.row <= a.c;
  if (i != 0u) ok = ok && rm_entry_in_bounds(from, S, R, R + 1u) && from.ordinal >= e0.ordinal && from.ordinal - e0.ordinal <= cap;
  if (!last)
  {
    to = rm_ld_entry(a.index, k);
    ok = ok && rm_entry_in_bounds(to, S, R, R + 1u) && rm_entry_behind(to, from) && to.ordinal - e0.ordinal <= cap;
  }
  RmDecArgs d = a.d;
  d.rec = a.d.rec - e0.ordinal;          // (used behind ok only: records [from.ordinal, to.ordinal) - e0.ordinal lie inside the table)
  d.maxRec = e0.ordinal + cap;
  uint64_t pos = from.offset;
  uint32_t row = from.row, n = from.ordinal;
  if (ok) ok = d_rm_walk_from<true>(d, sWin, lane, S, pos, row, n, from.kind == 1u, !last, to, nullptr, 0u, nullptr);
  if (lane != 0u) return;
  atomicMax(&a.d.ctrl[7], i);
  if (!ok) atomicOr(&a.d.ctrl[0], kRmIndex);
  else if (last || to.row >= a.r1)
  {
    a.d.ctrl[1] = (last ? n : to.ordinal) - e0.ordinal;
    if (last) a.d.ctrl[2] = (uint32_t)pos;
    a.d.ctrl[8] = 1u;
  }
}

// The waves that walked are 0 .. ctrl[7]; they are the stretches e0 .. the one that reaches r1 without a gap exactly if every wave behind them found nothing
// to do and one of them left the record count.
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_rm_expand_range(RmRangeArgs a)
{
  uint32_t status = a.d.ctrl[0];
  if (status == kRmDone && (a.d.ctrl[8] == 0u || a.d.ctrl[7] >= a.d.ctrl[6])) status = kRmIndex;
  if (blockIdx.x == 0u && threadIdx.x == 0u)
  {
    a.d.ctrl[5] = status;
    *a.d.status = status;
  }
  if (status != kRmDone) return;
  RmDecArgs d = a.d;
  d.ranks = a.d.ranks - (uint64_t)a.c * 16u;   // row c at the rank buffer's start
  d.rows = a.r1;
  const uint32_t lane = threadIdx.x & 63u, row0 = a.c + (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;
  if (blockIdx.x == 0u && a.r1 == a.d.rows) d_rm_expand_tail(d, threadIdx.x);
  if (row0 >= a.r1) return;
  d_rm_expand(d, row0, lane);
}

// Pass B from the checkpoint's lists (start = nullptr: from the identity): k_mmtf_scan_dec<16>'s loop (kept apart from it, so that that kernel stays
// the code it is).
template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_rm_range_scan(MmtfArgs a, const uint8_t *start)
{
  __shared__ uint32_t sCur[2][64];
  const uint32_t lane = threadIdx.x, col = blockIdx.x, S = a.S;
  uint32_t cur = start != nullptr ? ld32(start + col * 256u + lane * 4u) : 0x03020100u + 0x04040404u * lane;
  auto slot_of = [&](uint32_t s) -> uint32_t * { return rm_table_slot(a.table, s, col) + lane * 64u; };   // dword `lane` of the list: entries 4 lane .. 4 lane + 3
  constexpr uint32_t kBatch = 8;
  uint32_t p[kBatch], q[kBatch];
#pragma unroll
  for (uint32_t u = 0; u < kBatch; u++) p[u] = (u + 1u < S) ? *slot_of(u) : 0u;
  uint32_t flip = 0;
  for (uint32_t s0 = 0; s0 < S; s0 += kBatch)
  {
#pragma unroll
    for (uint32_t u = 0; u < kBatch; u++) q[u] = (s0 + kBatch + u + 1u < S) ? *slot_of(s0 + kBatch + u) : 0u;   // in flight during this batch
#pragma unroll
    for (uint32_t u = 0; u < kBatch; u++)
    {
      const uint32_t s = s0 + u;
      if (s < S)
      {
        *slot_of(s) = cur;
        if (s + 1u < S)
        {
          sCur[flip][lane] = cur;
          __syncthreads();
          const uint8_t *c = (const uint8_t *)sCur[flip];
          const uint32_t P = p[u];
          cur = (uint32_t)c[P & 0xFFu] | ((uint32_t)c[(P >> 8) & 0xFFu] << 8) | ((uint32_t)c[(P >> 16) & 0xFFu] << 16) | ((uint32_t)c[P >> 24] << 24);
          flip ^= 1u;
        }
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < kBatch; u++) p[u] = q[u];
  }
}

// Pass C: k_mmtf_rows<16, true, true> with segment 0 run from the checkpoint's lists.
template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_rm_range_rows(MmtfArgs a, const uint8_t *start)
{
  __shared__ uint32_t sList[kMmtfGroupDwords];
  __shared__ __attribute__((aligned(16))) uint8_t sTile[1024];
  const uint32_t lane = threadIdx.x, g = blockIdx.x;
  const uint32_t seg = (g * 64u + lane) / 16u, col = lane % 16u;
  const bool valid = seg < a.S;
  const uint32_t firstRow = valid ? seg * a.R : 0u;
  const uint32_t segRows = valid ? umin(a.R, a.rows - firstRow) : 0u;
  MmtfList L;
  L.lds = sList + lane;
  if (valid && seg != 0u) L.load(a.table + (uint64_t)g * kMmtfGroupDwords + lane);
  else if (valid && start != nullptr) rm_list_load_plain(L, start + col * 256u);
  else L.identity();
  uint32_t K = 0;
  d_mmtf_rows<16, true, true>(L, K, a.in + (uint64_t)firstRow * 16u, a.out + (uint64_t)firstRow * 16u, segRows, (a.R + 15u) / 16u, col, sTile + (lane / 16u) * 256u);
  if (valid && seg == a.S - 1u)
  {
    const uint32_t i = a.rows * 16u + col;   // the tail: column `col`'s list as it stands behind the last row
    if (i < a.size) a.out[i] = (uint8_t)L.at(a.in[i]);
  }
}

// from[0, length) to the caller's buffer, 16 bytes a lane, behind a DONE verdict only
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_rm_range_copy(const uint8_t *__restrict__ from, uint8_t *__restrict__ to, uint64_t length, const uint32_t *__restrict__ ctrl)
{
  if (ctrl[5] != kRmDone) return;
  for (uint64_t b = ((uint64_t)blockIdx.x * 256u + threadIdx.x) * 16u; b < length; b += (uint64_t)gridDim.x * 4096u)
  {
    if (b + 16u <= length) st128(to + b, ld128(from + b));
    else
      for (uint64_t k = b; k < length; k++) to[k] = from[k];
  }
}

}   // namespace hsrle
