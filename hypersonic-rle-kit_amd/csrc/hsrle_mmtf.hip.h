// hsrle_mmtf.hip.h -- the multi-move-to-front transforms of the reference (src/rle.h:420-438; src/mmtf.c, src/bit_mmtf.c) for gfx950.
//
// mmtf128 / mmtf256: byte i of the first rows * W bytes (W = 16 / 32) belongs to column i % W; every column owns a move-to-front list
// that starts as 0 .. 255; encode writes the byte's rank in its column's list, decode the symbol at that rank, both move it to the front.
// The n % W bytes behind the last row are looked up in the lists as they stand, without an update.
//
// A column is one sequential chain over the whole input.  Both directions are prefix computations over SEGMENTS of R rows:
//   pass A  k_mmtf_rows<W, DEC, false>   one lane per (segment, column), segments 0 .. S - 2, list = identity:
//             decode: the MTF of the ranks applied to position ids -- the permutation P the segment applies to ANY incoming list
//                     (after[i] = before[P[i]]); it does not depend on the list's contents
//             encode: the list after the segment from identity F and the number K of distinct symbols; F[0 .. K) are they, most recent
//                     first.  A symbol is new exactly when its rank is >= the number seen so far (unseen symbols stay behind the seen
//                     ones in identity order), so K needs no set.
//   pass B  k_mmtf_scan_dec / _enc<W>    one wave per column, 4 list entries per lane, one segment per step: the exclusive scan of the
//             compositions (decode: cur[P[i]], an LDS gather; encode: F[0 .. K) followed by cur without them, order kept -- stamps in
//             LDS, ballots for the kept entries' places).  In place: slot s then holds the list in front of segment s.
//   pass C  k_mmtf_rows<W, DEC, true>    every lane runs its segment from its true start list and writes the output; the lanes of the
//             last segment also look up the tail.
// State table: wave g of passes A / C owns 16 KiB, entry k of lane l in dword (k / 4) * 64 + l -- the layout of the lists in LDS, so a
// list moves between LDS and the table in 64 coalesced dword accesses and lanes asking for entry k hit different banks.
// List in a lane: dword 0 (ranks 0 .. 3) lives in a REGISTER, dwords 1 .. 63 in LDS.  A step searches and shifts in one sweep
// (d' = d << 8 | carry): ranks 0 .. 3 cost no LDS access, rank r costs r / 4 read-modify-writes, and a wave's step costs its slowest lane's.
// Rows reach the lanes through LDS: per 16 rows every lane loads 16 bytes of its segment's tile and reads its column from the tile, the
// ranks / symbols go back the same way and leave in 16-byte stores.
//
// bitmmtf8 / bitmmtf16: encode out[i] = in[i] ^ in[i - 1] on bytes / little-endian 16 bit words (element-wise, one element of halo);
// decode is the inclusive prefix XOR: XOR of every chunk, exclusive scan of the chunk values, apply (a wave per chunk).  An odd last byte
// of bitmmtf16 is copied.
#pragma once

#include "hsrle_common.hip.h"

namespace hsrle {

constexpr uint32_t kMmtfGroupBytes = 16384u;   // state of the 64 lanes of one wave
constexpr uint32_t kMmtfGroupDwords = 4096u;

// d with the bytes below b moved up by one and c at byte 0; the bytes above b stay (b = 0 .. 3)
__device__ __forceinline__ uint32_t mmtf_insert(uint32_t d, uint32_t c, uint32_t b)
{
  const uint32_t low = 0xFFFFFFFFu >> (8u * (3u - b));
  return (((d << 8) | c) & low) | (d & ~low);
}

// One lane's list: head = entries 0 .. 3, lds[j * 64] = entries 4j .. 4j + 3 (j = 1 .. 63; lds already points at the lane's column of dwords).
struct MmtfList
{
  uint32_t head;
  uint32_t *lds;

  __device__ __forceinline__ void identity()
  {
    head = 0x03020100u;
    for (uint32_t j = 1; j < 64u; j++) lds[j * 64u] = 0x03020100u + 0x04040404u * j;
  }
  __device__ __forceinline__ void load(const uint32_t *slot)   // slot: the lane's dword 0 in the table
  {
    head = slot[0];
    for (uint32_t j = 1; j < 64u; j++) lds[j * 64u] = slot[j * 64u];
  }
  __device__ __forceinline__ void store(uint32_t *slot) const
  {
    slot[0] = head;
    for (uint32_t j = 1; j < 64u; j++) slot[j * 64u] = lds[j * 64u];
  }
  // rank of x, x moved to the front
  __device__ __forceinline__ uint32_t encode(uint32_t x)
  {
    const uint32_t xx = x * 0x01010101u;
    uint32_t d = head, m = zero_bytes(d ^ xx);
    if (m)
    {
      const uint32_t b = first_set_byte(m);
      head = mmtf_insert(d, x, b);
      return b;
    }
    uint32_t carry = d >> 24;
    head = (d << 8) | x;
    for (uint32_t j = 1; j < 64u; j++)
    {
      d = lds[j * 64u];
      m = zero_bytes(d ^ xx);
      if (m)
      {
        const uint32_t b = first_set_byte(m);
        lds[j * 64u] = mmtf_insert(d, carry, b);
        return 4u * j + b;
      }
      lds[j * 64u] = (d << 8) | carry;
      carry = d >> 24;
    }
    return 255u;   // (not reached: the list is a permutation of 0 .. 255)
  }
  // symbol at rank k, moved to the front
  __device__ __forceinline__ uint32_t decode(uint32_t k)
  {
    const uint32_t b = k & 3u, jk = k >> 2;
    if (jk == 0u)
    {
      const uint32_t x = (head >> (8u * b)) & 0xFFu;
      head = mmtf_insert(head, x, b);
      return x;
    }
    uint32_t last = lds[jk * 64u];
    const uint32_t x = (last >> (8u * b)) & 0xFFu;
    uint32_t carry = head >> 24;
    head = (head << 8) | x;
    for (uint32_t j = 1; j < jk; j++)
    {
      const uint32_t d = lds[j * 64u];
      lds[j * 64u] = (d << 8) | carry;
      carry = d >> 24;
    }
    lds[jk * 64u] = mmtf_insert(last, carry, b);
    return x;
  }
  // the same without the move (the tail bytes)
  __device__ __forceinline__ uint32_t rank_of(uint32_t x) const
  {
    const uint32_t xx = x * 0x01010101u;
    uint32_t m = zero_bytes(head ^ xx);
    if (m) return first_set_byte(m);
    for (uint32_t j = 1; j < 64u; j++)
    {
      m = zero_bytes(lds[j * 64u] ^ xx);
      if (m) return 4u * j + first_set_byte(m);
    }
    return 255u;
  }
  __device__ __forceinline__ uint32_t at(uint32_t k) const
  {
    const uint32_t d = (k < 4u) ? head : lds[(k >> 2) * 64u];
    return (d >> (8u * (k & 3u))) & 0xFFu;
  }
};

struct MmtfArgs
{
  const uint8_t *in;
  uint8_t *out;
  uint32_t *table;   // groups * 4096 dwords
  uint32_t *counts;  // groups * 64 (encode: K per lane)
  uint32_t size, rows, R, S;   // rows = size / W, R rows per segment, S = ceil(rows / R) >= 1
};

// The row loop of a lane: `segRows` rows of column `col` from `src` through the list L, in tiles of 16 rows that reach the lanes through `tile` (the 16 rows
// of the lane's segment in LDS); FINAL: the ranks / symbols go to `dst` the same way.  `trips` is the same for every lane of the workgroup (the barriers
// are uniform); a lane without rows (segRows = 0) only keeps them.  K (encode, !FINAL): the number of distinct symbols so far.
template <int W, bool DEC, bool FINAL>
__device__ __forceinline__ void d_mmtf_rows(MmtfList &L, uint32_t &K, const uint8_t *src, uint8_t *dst, uint32_t segRows, uint32_t trips, uint32_t col, uint8_t *tile)
{
  u32x4 next = { 0u, 0u, 0u, 0u };
  if (segRows >= 16u) next = ld128(src + col * 16u);
  for (uint32_t t = 0; t < trips; t++)
  {
    const uint32_t r0 = t * 16u;
    const uint32_t cnt = (r0 < segRows) ? umin(16u, segRows - r0) : 0u;
    const bool full = cnt == 16u;
    const uint8_t *p = src + (uint64_t)r0 * W;
    uint8_t v[16];
    if (full) lds_st128(tile + col * 16u, next);
    if (r0 + 32u <= segRows) next = ld128(p + 16u * W + col * 16u);   // the next tile's share, in flight during this one's steps
    __syncthreads();
    if (full)
    {
#pragma unroll
      for (uint32_t j = 0; j < 16u; j++) v[j] = tile[j * W + col];
    }
    else
    {
#pragma unroll
      for (uint32_t j = 0; j < 16u; j++) v[j] = (j < cnt) ? p[j * W + col] : (uint8_t)0;
    }
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++)
    {
      if (j < cnt)
      {
        uint32_t o;
        if (DEC) o = L.decode(v[j]);
        else
        {
          o = L.encode(v[j]);
          if (!FINAL && o >= K) K++;
        }
        v[j] = (uint8_t)o;
      }
    }
    if (FINAL)
    {
      uint8_t *q = dst + (uint64_t)r0 * W;
      if (full)
      {
#pragma unroll
        for (uint32_t j = 0; j < 16u; j++) tile[j * W + col] = v[j];
      }
      else
      {
#pragma unroll
        for (uint32_t j = 0; j < 16u; j++)
          if (j < cnt) q[j * W + col] = v[j];
      }
      __syncthreads();
      if (full) st128(q + col * 16u, lds_ld128(tile + col * 16u));
      __syncthreads();
    }
    else
      __syncthreads();
  }
}

// Passes A (FINAL = false: segments 0 .. S - 2, from identity, leaves the state) and C (FINAL = true: from the table, writes the output).
template <int W, bool DEC, bool FINAL>
__global__ __launch_bounds__(64) void k_mmtf_rows(MmtfArgs a)
{
  __shared__ uint32_t sList[kMmtfGroupDwords];
  __shared__ __attribute__((aligned(16))) uint8_t sTile[1024];
  const uint32_t lane = threadIdx.x, g = blockIdx.x;
  const uint32_t seg = (g * 64u + lane) / (uint32_t)W, col = lane % (uint32_t)W;
  const uint32_t segs = FINAL ? a.S : a.S - 1u;
  const bool valid = seg < segs;
  const uint32_t firstRow = valid ? seg * a.R : 0u;
  const uint32_t segRows = valid ? umin(a.R, a.rows - firstRow) : 0u;
  MmtfList L;
  L.lds = sList + lane;
  uint32_t *slot = a.table + (uint64_t)g * kMmtfGroupDwords + lane;
  if (FINAL && valid && seg != 0u) L.load(slot); else L.identity();
  uint32_t K = 0;
  uint8_t *tile = sTile + (lane / (uint32_t)W) * 16u * (uint32_t)W;   // this segment's 16 rows
  d_mmtf_rows<W, DEC, FINAL>(L, K, a.in + (uint64_t)firstRow * W, a.out + (uint64_t)firstRow * W, segRows, (a.R + 15u) / 16u, col, tile);
  if (!FINAL)
  {
    if (valid)
    {
      L.store(slot);
      if (!DEC) a.counts[(uint64_t)g * 64u + lane] = K;
    }
  }
  else if (valid && seg == a.S - 1u)
  {
    const uint32_t i = a.rows * (uint32_t)W + col;   // the tail: byte `col` behind the last row, column `col`'s list as it stands
    if (i < a.size) a.out[i] = (uint8_t)(DEC ? L.at(a.in[i]) : L.rank_of(a.in[i]));
  }
}

// Pass B, decode: one wave per column; slot s <- the list in front of segment s.
template <int W>
__global__ __launch_bounds__(64) void k_mmtf_scan_dec(MmtfArgs a)
{
  __shared__ uint32_t sCur[2][64];
  const uint32_t lane = threadIdx.x, col = blockIdx.x, S = a.S;
  uint32_t cur = 0x03020100u + 0x04040404u * lane;
  auto slot_of = [&](uint32_t s) -> uint32_t * {
    const uint32_t id = s * (uint32_t)W + col;
    return a.table + (uint64_t)(id >> 6) * kMmtfGroupDwords + lane * 64u + (id & 63u);
  };
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

// Pass B, encode: after = F[0 .. K) followed by (before without those symbols, order kept).
template <int W>
__global__ __launch_bounds__(64) void k_mmtf_scan_enc(MmtfArgs a)
{
  __shared__ uint32_t sStamp[256];
  __shared__ uint32_t sNew[64];
  const uint32_t lane = threadIdx.x, col = blockIdx.x, S = a.S;
  uint32_t cur = 0x03020100u + 0x04040404u * lane;
  auto slot_of = [&](uint32_t s) -> uint32_t * {
    const uint32_t id = s * (uint32_t)W + col;
    return a.table + (uint64_t)(id >> 6) * kMmtfGroupDwords + lane * 64u + (id & 63u);
  };
  for (uint32_t i = lane; i < 256u; i += 64u) sStamp[i] = 0u;
  __syncthreads();
  constexpr uint32_t kBatch = 8;
  uint32_t p[kBatch], q[kBatch], pk[kBatch], qk[kBatch];
#pragma unroll
  for (uint32_t u = 0; u < kBatch; u++)
  {
    const bool have = u + 1u < S;
    p[u] = have ? *slot_of(u) : 0u;
    pk[u] = have ? a.counts[(uint64_t)u * W + col] : 0u;
  }
  uint8_t *nb = (uint8_t *)sNew;
  for (uint32_t s0 = 0; s0 < S; s0 += kBatch)
  {
#pragma unroll
    for (uint32_t u = 0; u < kBatch; u++)
    {
      const bool have = s0 + kBatch + u + 1u < S;
      q[u] = have ? *slot_of(s0 + kBatch + u) : 0u;
      qk[u] = have ? a.counts[(uint64_t)(s0 + kBatch + u) * W + col] : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < kBatch; u++)
    {
      const uint32_t s = s0 + u;
      if (s < S)
      {
        *slot_of(s) = cur;
        if (s + 1u < S)
        {
          const uint32_t F = p[u], K = umin(pk[u], 256u), stamp = s + 1u;
#pragma unroll
          for (uint32_t b = 0; b < 4u; b++)
          {
            const uint32_t f = (F >> (8u * b)) & 0xFFu;
            if (4u * lane + b < K) { sStamp[f] = stamp; nb[4u * lane + b] = (uint8_t)f; }
          }
          __syncthreads();
          uint32_t before = 0;
          bool keep[4];
#pragma unroll
          for (uint32_t b = 0; b < 4u; b++)
          {
            keep[b] = sStamp[(cur >> (8u * b)) & 0xFFu] != stamp;
            const uint64_t m = __ballot(keep[b]);
            before += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
          }
          uint32_t place = K + before;
#pragma unroll
          for (uint32_t b = 0; b < 4u; b++)
            if (keep[b])
            {
              if (place < 256u) nb[place] = (uint8_t)(cur >> (8u * b));
              place++;
            }
          __syncthreads();
          cur = sNew[lane];
          __syncthreads();
        }
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < kBatch; u++) { p[u] = q[u]; pk[u] = qk[u]; }
  }
}

// fewer than W bytes: no row, every byte is a tail byte on an identity list -- rank == symbol
template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_mmtf_copy_small(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint32_t n)
{
  if (threadIdx.x < n) out[threadIdx.x] = in[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------------------------
// bitmmtf.  E = element bytes (1 / 2), m = the bytes that belong to whole elements.

// out[b] = in[b] ^ in[b - E] (b >= E); 16 bytes per lane, the halo is a second load E bytes lower
template <int E>
__global__ __launch_bounds__(256) void k_bitmmtf_enc(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint32_t m, uint32_t size)
{
  const uint64_t pieces = ((uint64_t)m + 15u) / 16u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < pieces; i += (uint64_t)gridDim.x * 256u)
  {
    const uint64_t b = i * 16u;
    if (i != 0u && b + 16u <= m)
      st128(out + b, ld128(in + b) ^ ld128(in + b - E));
    else
      for (uint64_t k = b; k < m && k < b + 16u; k++) out[k] = (uint8_t)(in[k] ^ (k >= (uint64_t)E ? in[k - E] : 0));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && m < size) out[m] = in[m];
}

// inclusive prefix XOR of the elements inside 16 bytes; returns the piece's total in the low E bytes
template <int E>
__device__ __forceinline__ uint32_t bitmmtf_scan16(u32x4 &v)
{
  constexpr uint32_t kRep = (E == 1) ? 0x01010101u : 0x00010001u;
  constexpr uint32_t kTop = (E == 1) ? 24u : 16u;
  uint32_t carry = 0;
#pragma unroll
  for (int k = 0; k < 4; k++)
  {
    uint32_t d = v[k];
    if (E == 1) d ^= d << 8;
    d ^= d << 16;
    d ^= carry * kRep;
    carry = d >> kTop;
    v[k] = d;
  }
  return carry;
}
template <int E>
__device__ __forceinline__ uint32_t bitmmtf_fold(u32x4 v)
{
  uint32_t x = v[0] ^ v[1] ^ v[2] ^ v[3];
  x ^= x >> 16;
  if (E == 1) { x ^= x >> 8; return x & 0xFFu; }
  return x & 0xFFFFu;
}
// the lane's up-to-16 bytes of [lo, hi) at b, zeros behind (zero is neutral)
__device__ __forceinline__ u32x4 bitmmtf_load(const uint8_t *in, uint64_t b, uint32_t hi)
{
  u32x4 v = { 0u, 0u, 0u, 0u };
  if (b + 16u <= hi) return ld128(in + b);
  for (uint32_t k = 0; k < 16u && b + k < hi; k++) v[k >> 2] |= (uint32_t)in[b + k] << (8u * (k & 3u));
  return v;
}
__device__ __forceinline__ uint32_t wave_xor(uint32_t x)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x ^= __shfl_xor(x, o, 64);
  return x;
}

// XOR of the elements of chunk c (chunkBytes each, the last one shorter): a wave per chunk
template <int E>
__global__ __launch_bounds__(64) void k_bitmmtf_reduce(const uint8_t *__restrict__ in, uint32_t m, uint32_t chunkBytes, uint32_t *__restrict__ vals)
{
  const uint64_t lo64 = (uint64_t)blockIdx.x * chunkBytes;
  const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)(lo64 + chunkBytes < m ? lo64 + chunkBytes : m);
  uint32_t x = 0;
  for (uint64_t b = (uint64_t)lo + threadIdx.x * 16u; b < hi; b += 1024u) x ^= bitmmtf_fold<E>(bitmmtf_load(in, b, hi));
  x = wave_xor(x);
  if (threadIdx.x == 0) vals[blockIdx.x] = x;
}

// exclusive prefix XOR of vals[0, n) in place: one workgroup, a run of values per thread
template <int UNUSED = 0>
__global__ __launch_bounds__(1024) void k_bitmmtf_scan(uint32_t *__restrict__ vals, uint32_t n)
{
  __shared__ uint32_t sWave[16];
  const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u;
  const uint64_t lo = (uint64_t)t * per;
  const uint64_t hi = lo + per < n ? lo + per : n;
  uint32_t x = 0;
  for (uint64_t i = lo; i < hi; i++) x ^= vals[i];
  uint32_t inc = x;   // inclusive scan inside the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1)
  {
    const uint32_t y = __shfl_up(inc, o, 64);
    if ((t & 63u) >= (uint32_t)o) inc ^= y;
  }
  if ((t & 63u) == 63u) sWave[t >> 6] = inc;
  __syncthreads();
  uint32_t carry = inc ^ x;
  for (uint32_t w = 0; w < (t >> 6); w++) carry ^= sWave[w];
  for (uint64_t i = lo; i < hi; i++)
  {
    const uint32_t v = vals[i];
    vals[i] = carry;
    carry ^= v;
  }
}

// out = inclusive prefix XOR of chunk c, started from vals[c] (vals == nullptr: one chunk, from 0): a wave per chunk, 1 KiB per trip
template <int E>
__global__ __launch_bounds__(64) void k_bitmmtf_apply(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, uint32_t m, uint32_t size, uint32_t chunkBytes,
                                                     const uint32_t *__restrict__ vals)
{
  constexpr uint32_t kRep = (E == 1) ? 0x01010101u : 0x00010001u;
  const uint32_t lane = threadIdx.x;
  const uint64_t lo64 = (uint64_t)blockIdx.x * chunkBytes;
  const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)(lo64 + chunkBytes < m ? lo64 + chunkBytes : m);
  uint32_t carry = vals ? vals[blockIdx.x] : 0u;
  for (uint64_t base = lo; base < hi; base += 1024u)
  {
    const uint64_t b64 = base + lane * 16u;
    const bool any = b64 < hi;
    u32x4 v = { 0u, 0u, 0u, 0u };
    if (any) v = bitmmtf_load(in, b64, hi);
    const uint32_t total = bitmmtf_scan16<E>(v);
    uint32_t inc = total;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
    {
      const uint32_t y = __shfl_up(inc, o, 64);
      if (lane >= (uint32_t)o) inc ^= y;
    }
    const uint32_t pre = (carry ^ inc ^ total) * kRep;
    carry ^= __shfl(inc, 63, 64);
    if (any)
    {
      v[0] ^= pre; v[1] ^= pre; v[2] ^= pre; v[3] ^= pre;
      if (b64 + 16u <= hi) st128(out + b64, v);
      else
        for (uint32_t k = 0; b64 + k < hi; k++) out[b64 + k] = (uint8_t)(v[k >> 2] >> (8u * (k & 3u)));
    }
  }
  if (blockIdx.x == 0 && lane == 0 && m < size) out[m] = in[m];
}

}   // namespace hsrle
