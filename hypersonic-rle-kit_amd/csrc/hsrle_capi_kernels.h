// hsrle_capi_kernels.h -- part of hsrle_capi.hip: the kernels this translation unit owns (container assembly, block hash, synthetic workloads), the scan's host side
#pragma once
#include "hsrle_capi_host.h"

namespace hsrle {

constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanTile = kScanThreads * kScanItems; // 2048 elements per workgroup

template <int THREADS = kScanThreads>
__device__ __forceinline__ uint64_t wg_exclusive_scan_u64(uint64_t v, uint64_t *total)
{
  // wave scan by shuffles, then a scan of the wave totals through LDS
  __shared__ uint64_t waveTotals[THREADS / 64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint64_t y = __shfl_up(x, d, 64);
    if ((int)lane >= d) x += y;
  }
  if (lane == 63u) waveTotals[wave] = x;
  __syncthreads();
  uint64_t base = 0, all = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; w++)
  {
    const uint64_t t = waveTotals[w];
    if ((uint32_t)w < wave) base += t;
    all += t;
  }
  __syncthreads();
  *total = all;
  return base + x - v;
}

// sums[wg] = sum of in[wg * 2048 .. +2048)
template <typename TIN>
__global__ __launch_bounds__(kScanThreads) void k_tile_sums(const TIN *__restrict__ in, uint64_t n, uint64_t *__restrict__ sums)
{
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile;
  uint64_t acc = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; k++)
  {
    const uint64_t idx = base + (uint64_t)k * kScanThreads + threadIdx.x;
    if (idx < n) acc += (uint64_t)in[idx];
  }
  uint64_t total;
  wg_exclusive_scan_u64(acc, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// out[i] = tileBase[wg] + exclusive prefix of in within the tile; out[n] = grand total when writeTotal.
// `in` and `out` may alias (in-place scan of a sums level): every thread reads its items before it writes them.
// `carry` (may be null): a device value added to every result -- the chunked compression scans chunk after chunk, each starting at the
// total of the chunks in front of it (which is the out[n] the previous chunk's scan wrote: carry may alias out[0]).
template <typename TIN>
__global__ __launch_bounds__(kScanThreads) void k_tile_scan(const TIN *in, uint64_t n, const uint64_t *tileBase, uint64_t *out, int writeTotal, const uint64_t *carry = nullptr)
{
  const uint64_t base = (uint64_t)blockIdx.x * kScanTile + (uint64_t)threadIdx.x * kScanItems;
  uint64_t v[kScanItems];
  uint64_t acc = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; k++)
  {
    v[k] = (base + k < n) ? (uint64_t)in[base + k] : 0;
    acc += v[k];
  }
  uint64_t total;
  const uint64_t carried = carry ? *carry : 0;
  uint64_t run = wg_exclusive_scan_u64(acc, &total) + (tileBase ? tileBase[blockIdx.x] : 0) + carried;
#pragma unroll
  for (int k = 0; k < kScanItems; k++)
  {
    if (base + k < n) out[base + k] = run;
    run += v[k];
  }
  if (writeTotal && n > 0 && base <= n - 1 && n - 1 < base + kScanItems) // the thread that owns the last element
    out[n] = run;
}

// one wave per block: copy the slot stream to its place in the payload (destination-aligned 16-byte stores)
__global__ __launch_bounds__(256) void k_compact(const uint8_t *__restrict__ slots, uint32_t slotStride, const uint64_t *__restrict__ offsets,
                                                 uint8_t *__restrict__ payload, uint32_t nBlocks)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = xcd_tile(blockIdx.x, gridDim.x) * 4u + (threadIdx.x >> 6);   // XCD-aware tile order (hsrle_common.hip.h)
  if (b >= nBlocks)
    return;

  const uint64_t off = offsets[b];
  const uint32_t size = (uint32_t)(offsets[b + 1] - off);
  const uint8_t *src = slots + (uint64_t)b * slotStride;
  uint8_t *dst = payload + off;

  uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
  if (head > size) head = size;
  if (lane < head) dst[lane] = src[lane];

  const uint32_t body = (size - head) & ~15u;
  for (uint32_t k = lane * 16u; k < body; k += 64u * 16u)
    st128(dst + head + k, ld128(src + head + k));

  const uint32_t tail = size - head - body;
  if (lane < tail) dst[head + body + lane] = src[head + body + lane];
}

struct ContainerHeader
{
  char magic[8];
  uint32_t version, codec;
  uint64_t uncompressedSize;
  uint32_t blockSize, blockCount;
  uint64_t payloadSize, totalSize;
  uint8_t reserved[16];
};
static_assert(sizeof(ContainerHeader) == HSRLE_CONTAINER_HEADER_SIZE, "container header is 64 bytes");

__device__ __forceinline__ void finish_container(uint8_t *__restrict__ container, uint32_t codec, uint64_t U, uint32_t B, uint32_t nBlocks, uint64_t payloadSize);

__global__ void k_finish_container(uint8_t *__restrict__ container, uint32_t codec, uint64_t U, uint32_t B, uint32_t nBlocks)
{
  // offsets[nBlocks] was written by the scan; fill the header and the zero tail pad
  const uint64_t *offsets = (const uint64_t *)(container + HSRLE_CONTAINER_HEADER_SIZE);
  finish_container(container, codec, U, B, nBlocks, offsets[nBlocks]);
}

// Small containers (up to kScanSmallMax blocks): the size scan in ONE launch -- every workgroup first adds up all sizes in front of its tile
// itself (at most 128 KB of coalesced reads from L2: cheaper than a launch), then scans its tile; the last one writes the container's header
// and tail pad.  One launch where k_tile_sums + 2 x k_tile_scan + k_finish_container were four, ~5 us each on a call of 150 (BASELINE
// config 3).  (A version with one workgroup of 1024 threads took 17 us: its loads and stores were strided by thread.)
constexpr uint32_t kScanSmallMax = 262144u;   // (128 workgroups, the last of which adds up 1 MiB of sizes: still cheaper than two more launches)
__global__ __launch_bounds__(kScanThreads) void k_scan_small_finish(const uint32_t *__restrict__ sizes, uint32_t n, uint64_t *__restrict__ out, uint8_t *__restrict__ container, uint32_t codec,
                                                                    uint64_t U, uint32_t B)
{
  const uint32_t tileFirst = blockIdx.x * (uint32_t)kScanTile;
  // sum of sizes[0, tileFirst): 16 bytes per thread and load, four loads in flight (tileFirst is a multiple of 2048)
  uint64_t before = 0;
  for (uint32_t i = threadIdx.x * 4u; i < tileFirst; i += 4u * 4u * kScanThreads)
  {
    u32x4 q[4];
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++)
    {
      const uint32_t at = i + j * 4u * kScanThreads;
      q[j] = *(const u32x4 *)(sizes + (at < tileFirst ? at : 0u));
      if (at >= tileFirst) q[j] = u32x4{ 0, 0, 0, 0 };
    }
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) before += (uint64_t)q[j].x + q[j].y + q[j].z + q[j].w;
  }
  uint64_t beforeAll;
  (void)wg_exclusive_scan_u64(before, &beforeAll);

  const uint32_t base = tileFirst + threadIdx.x * (uint32_t)kScanItems;
  static_assert(kScanItems == 8, "two 16-byte loads per thread");
  const uint32_t lastVec = (n - 1u) >> 2;                                // (the size table is padded to 256 bytes: the vector that holds size n - 1 is readable)
  const uint32_t v0 = base >> 2, v1 = v0 + 1u;
  const u32x4 qa = *(const u32x4 *)(sizes + 4u * (v0 < lastVec ? v0 : lastVec)), qb = *(const u32x4 *)(sizes + 4u * (v1 < lastVec ? v1 : lastVec));
  const uint32_t x[8] = { qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w };
  uint32_t v[8];
  uint64_t acc = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) { v[k] = (base + (uint32_t)k < n) ? x[k] : 0u; acc += v[k]; }
  uint64_t total;
  uint64_t run = wg_exclusive_scan_u64(acc, &total) + beforeAll;
#pragma unroll
  for (int k = 0; k < 8; k++)
  {
    if (base + (uint32_t)k < n) out[base + (uint32_t)k] = run;
    run += v[k];
  }
  if (blockIdx.x == gridDim.x - 1u)
  {
    if (threadIdx.x == 0) out[n] = beforeAll + total;
    if (container != nullptr) finish_container(container, codec, U, B, n, beforeAll + total);   // (nullptr: a scan only -- scan_sizes)
  }
}

__device__ __forceinline__ void finish_container(uint8_t *__restrict__ container, uint32_t codec, uint64_t U, uint32_t B, uint32_t nBlocks, uint64_t payloadSize)
{
  const uint64_t payloadStart = HSRLE_CONTAINER_HEADER_SIZE + 8ull * ((uint64_t)nBlocks + 1ull);

  if (threadIdx.x == 0)
  {
    ContainerHeader h;
    const char m[8] = { 'H', 'S', 'R', 'L', 'E', 'K', 'I', 'T' };
    for (int k = 0; k < 8; k++) h.magic[k] = m[k];
    h.version = 1;
    h.codec = codec;
    h.uncompressedSize = U;
    h.blockSize = B;
    h.blockCount = nBlocks;
    h.payloadSize = payloadSize;
    h.totalSize = payloadStart + payloadSize + HSRLE_CONTAINER_TAIL_PAD;
    for (int k = 0; k < 16; k++) h.reserved[k] = 0;
    *(ContainerHeader *)container = h;
  }

  if (threadIdx.x < HSRLE_CONTAINER_TAIL_PAD)
    container[payloadStart + payloadSize + threadIdx.x] = 0;
}

// ------------------------------------------------------------------------------------------------------------------
// 64 bit hash of every block stream of a container (include/hsrle.h: hsrle_hash_blocks_dev_async): what the big-config manifests pin
// (tests/golden/big/, minted from the compiled reference) -- every block of an 8 GiB container is compared, not a sample.

__device__ __forceinline__ uint64_t rotl64(uint64_t v, int sh) { return (v << sh) | (v >> (64 - sh)); }

__global__ __launch_bounds__(256) void k_hash_blocks(const uint8_t *__restrict__ payload, const uint64_t *__restrict__ offsets, uint64_t payloadBytes, uint32_t firstBlock,
                                                     uint32_t blockCount, uint64_t *__restrict__ out)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= blockCount) return;
  const uint64_t off0 = offsets[firstBlock + i], off1 = offsets[firstBlock + i + 1u];
  if (off0 > off1 || off1 > payloadBytes) { out[i] = 0; return; }
  const uint8_t *p = payload + off0;
  const uint64_t len = off1 - off0;
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (len * 0xD6E8FEB86659FD93ull);
  uint64_t k = 0;
  for (; k + 8 <= len; k += 8)
    h = rotl64(h ^ ld64(p + k), 27) * 0x9E3779B97F4A7C15ull + 0x165667B19E3779F9ull;
  if (k < len)
  {
    uint64_t w = 0;
    for (uint32_t j = 0; k + j < len; j++) w |= (uint64_t)p[k + j] << (8u * j);
    h = rotl64(h ^ w, 27) * 0x9E3779B97F4A7C15ull + 0x165667B19E3779F9ull;
  }
  out[i] = h ^ (h >> 31);
}

// ------------------------------------------------------------------------------------------------------------------
// synthetic workloads.  One lane generates one 64 KiB chunk; chunks are independent so the same
// bytes can be produced on the CPU (oracle/hsrle_synth.c, tests/hsrle_testlib.py:synth_chunk_py) for any slice.

constexpr uint32_t kSynthChunk = 65536u;

__device__ __forceinline__ uint64_t splitmix64(uint64_t &state)
{
  state += 0x9E3779B97F4A7C15ull;
  uint64_t z = state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(64) void k_synth(int kind, int S, uint64_t seed, uint8_t *__restrict__ out, uint64_t size)
{
  const uint64_t chunk = (uint64_t)blockIdx.x * 64u + threadIdx.x;
  const uint64_t start = chunk * kSynthChunk;
  if (start >= size)
    return;

  const uint32_t len = (uint32_t)((size - start) < kSynthChunk ? (size - start) : kSynthChunk);
  uint8_t *o = out + start;
  uint64_t st = seed * 0x9E3779B97F4A7C15ull + chunk * 0xD1B54A32D192ED03ull + (uint64_t)kind;
  uint32_t at = 0;

  if (kind == HSRLE_SYNTH_RUNS)
  {
    while (at < len)
    {
      uint64_t r = splitmix64(st);
      uint32_t L = 1u + (uint32_t)(r % 63u);
      for (uint32_t k = 0; k < L; k += 8)
      {
        const uint64_t v = splitmix64(st);
        for (uint32_t j = 0; j < 8 && k + j < L; j++)
          if (at + k + j < len) o[at + k + j] = (uint8_t)(v >> (8 * j));
      }
      at += L;

      r = splitmix64(st);
      const uint32_t R = 2u + (uint32_t)(r % 62u);
      uint8_t sym[16];
      for (int k = 0; k < S; k += 8)
      {
        const uint64_t v = splitmix64(st);
        for (int j = 0; j < 8 && k + j < S; j++) sym[k + j] = (uint8_t)(v >> (8 * j));
      }
      for (uint32_t k = 0; k < R * (uint32_t)S && at + k < len; k++)
        o[at + k] = sym[k % (uint32_t)S];
      at += R * (uint32_t)S;
    }
  }
  else
  {
    const uint8_t vals[6] = { 0x01, 0x02, 0x03, 0xFF, 0xFE, 0x04 };
    while (at < len)
    {
      uint64_t r = splitmix64(st);
      const uint32_t Z = (((r >> 32) & 3u) == 0u) ? 40u + (uint32_t)(r % 120u) : 10u + (uint32_t)(r % 16u);
      for (uint32_t k = 0; k < Z && at + k < len; k++) o[at + k] = 0;
      at += Z;
      r = splitmix64(st);
      const uint32_t Bn = 1u + (uint32_t)(r % 9u);
      for (uint32_t k = 0; k < Bn && at + k < len; k++) o[at + k] = vals[(r >> (8 + 4 * k)) % 6u];
      at += Bn;
    }
  }
}

// the sum levels of a scan over up to `count` values: tiles per level, and where each level's sums (+ 1 total) live in a workspace
struct ScanLevels
{
  uint64_t t1, t2, t3, offL1, offL2, offL3;
  void lay_out(uint64_t count, uint64_t &at)
  {
    t1 = (count + kScanTile - 1) / kScanTile;
    t2 = (t1 + kScanTile - 1) / kScanTile;
    t3 = (t2 + kScanTile - 1) / kScanTile;
    offL1 = at; at += align_up((t1 + 1) * 8ull, 256);
    offL2 = at; at += align_up((t2 + 1) * 8ull, 256);
    offL3 = at; at += align_up((t3 + 1) * 8ull, 256);
  }
};

// exclusive scan of `n` values (u32 at level 0) into out[0..n] (out[n] = total) using the pre-planned sum levels; `carry` as in k_tile_scan
static hipError_t scan_sizes(const uint32_t *sizes, uint64_t n, uint64_t *out, uint8_t *ws, const ScanLevels &w, hipStream_t st, const uint64_t *carry = nullptr)
{
  uint64_t *l1 = (uint64_t *)(ws + w.offL1), *l2 = (uint64_t *)(ws + w.offL2), *l3 = (uint64_t *)(ws + w.offL3);
  const uint64_t t1 = (n + kScanTile - 1) / kScanTile, t2 = (t1 + kScanTile - 1) / kScanTile, t3 = (t2 + kScanTile - 1) / kScanTile;
  if (carry == nullptr && n != 0 && n <= kScanSmallMax && (((uintptr_t)sizes) & 15u) == 0u)
  {
    // small tables (the split encode's flags and chunk sizes, small containers): one launch (k_scan_small_finish without the finish)
    hipLaunchKernelGGL(k_scan_small_finish, dim3((uint32_t)t1), dim3(kScanThreads), 0, st, sizes, (uint32_t)n, out, (uint8_t *)nullptr, 0u, 0ull, 0u);
    return hipGetLastError();
  }

  if (t1 > 1)
  {
    hipLaunchKernelGGL(k_tile_sums<uint32_t>, dim3((uint32_t)t1), dim3(kScanThreads), 0, st, sizes, n, l1);
    if (t2 > 1)
    {
      hipLaunchKernelGGL(k_tile_sums<uint64_t>, dim3((uint32_t)t2), dim3(kScanThreads), 0, st, l1, t1, l2);
      if (t3 > 1)
        return hipErrorInvalidValue; // > 2048^3 blocks: not representable anyway
      hipLaunchKernelGGL(k_tile_scan<uint64_t>, dim3(1), dim3(kScanThreads), 0, st, l2, t2, (const uint64_t *)nullptr, l3, 0, (const uint64_t *)nullptr);
      hipLaunchKernelGGL(k_tile_scan<uint64_t>, dim3((uint32_t)t2), dim3(kScanThreads), 0, st, l1, t1, l3, l1, 0, (const uint64_t *)nullptr);
    }
    else
    {
      hipLaunchKernelGGL(k_tile_scan<uint64_t>, dim3(1), dim3(kScanThreads), 0, st, l1, t1, (const uint64_t *)nullptr, l1, 0, (const uint64_t *)nullptr);
    }
    hipLaunchKernelGGL(k_tile_scan<uint32_t>, dim3((uint32_t)t1), dim3(kScanThreads), 0, st, sizes, n, l1, out, 1, carry);
  }
  else
  {
    hipLaunchKernelGGL(k_tile_scan<uint32_t>, dim3(1), dim3(kScanThreads), 0, st, sizes, n, (const uint64_t *)nullptr, out, 1, carry);
  }

  return hipGetLastError();
}

} // namespace hsrle
