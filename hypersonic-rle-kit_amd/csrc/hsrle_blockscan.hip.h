// hsrle_blockscan.hip.h -- what the two stream-block containers of include/hsrle.h section 5 ("HSRLESHB": hsrle_rle8shb.hip.h, "HSRLEMFB":
// hsrle_rle8mmtfb.hip.h) share on the device: the layout (64 header bytes, u64 offset[blockCount + 1], the block streams back to back, 32 zero bytes),
// the words of a slot that the group scan reads and writes, and the group scan itself.
//
// Blocks go through in GROUPS of `count` (the host loops and only enqueues); a block of the group owns slot `j` of the workspace, whose first words are
//   [0] in: the block's stream cannot be written, out: 1 = the container does not fit (gates the block's write pass off)   [3] in: the stream's size
//   [10], [11] out: the stream's offset in the payload
#pragma once

#include "hsrle_common.hip.h"

namespace hsrle {

constexpr uint32_t kBlkHeader = 64u, kBlkPad = 32u;
constexpr uint32_t kBlkScanThreads = 1024u;
constexpr uint32_t kBlkFail = 0u, kBlkStreamSize = 3u, kBlkAtLo = 10u, kBlkAtHi = 11u;
constexpr uint32_t kBlkDone = 0u, kBlkCapacity = 2u;   // == HSRLE_RLE8_SH_* == HSRLE_RLE8_MMTF_* (include/hsrle.h)

struct BlkScanArgs
{
  uint8_t *out;          // the container
  uint8_t *slots;        // slot 0
  uint32_t *run;         // [0], [1] payload bytes of the groups before this one, [2] 1: the container does not fit
  uint64_t *outSize;
  uint32_t *status;
  uint64_t inSize, outCap, slotStride, magic;
  uint32_t blockSize, blockCount, first, count, last;   // blocks [first, first + count) of blockCount; last: the last group
};

// Inside a kernel the passes of a block meet through global memory of the SAME workgroup: a device-scope fence and a barrier stand between them.
__device__ __forceinline__ void blk_pass_edge()
{
  __threadfence();
  __syncthreads();
}

template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_blk_begin(uint32_t *words, uint32_t count)
{
  if (threadIdx.x < count) words[threadIdx.x] = 0u;
}

// ONE workgroup of kBlkScanThreads: exclusive scan of the group's stream sizes onto the running payload size; the offset table; whether the group still
// fits; behind the last group the header, the pad, the size word and the status (or the struck magic).  sSum: kBlkScanThreads words of LDS.
__device__ __forceinline__ void d_blk_scan(const BlkScanArgs &g, uint64_t *sSum)
{
  const uint32_t t = threadIdx.x, per = (g.count + kBlkScanThreads - 1u) / kBlkScanThreads;
  const uint32_t lo = umin(t * per, g.count), hi = umin(lo + per, g.count);
  const uint64_t base = (uint64_t)g.run[0] | (uint64_t)g.run[1] << 32;
  int bad = g.run[2] != 0u;
  uint64_t sum = 0u;
  for (uint32_t j = lo; j < hi; j++)
  {
    const uint32_t *ctrl = (const uint32_t *)(g.slots + (uint64_t)j * g.slotStride);
    if (ctrl[kBlkFail] != 0u) bad = 1; else sum += ctrl[kBlkStreamSize];
  }
  bad = __syncthreads_or(bad);   // (every thread has read run[] in front of this barrier)
  sSum[t] = sum;
  __syncthreads();
  for (uint32_t d = 1u; d < kBlkScanThreads; d <<= 1)
  {
    const uint64_t v = t >= d ? sSum[t - d] : 0u;
    __syncthreads();
    sSum[t] += v;
    __syncthreads();
  }
  const uint64_t total = sSum[kBlkScanThreads - 1u], payload = (uint64_t)kBlkHeader + 8ull * ((uint64_t)g.blockCount + 1u);
  const bool fail = bad != 0 || payload + base + total + kBlkPad > g.outCap;
  uint64_t at = base + sSum[t] - sum;
  for (uint32_t j = lo; j < hi; j++)
  {
    uint32_t *ctrl = (uint32_t *)(g.slots + (uint64_t)j * g.slotStride);
    if (fail) { ctrl[kBlkFail] = 1u; continue; }   // (gates the block's write pass off)
    st64(g.out + kBlkHeader + 8ull * (g.first + j), at);   // (the host has seen that header, table and pad fit)
    ctrl[kBlkAtLo] = (uint32_t)at;
    ctrl[kBlkAtHi] = (uint32_t)(at >> 32);
    at += ctrl[kBlkStreamSize];
  }
  if (t != 0u) return;
  const uint64_t payloadSize = base + total;
  g.run[0] = (uint32_t)payloadSize;
  g.run[1] = (uint32_t)(payloadSize >> 32);
  g.run[2] = fail ? 1u : 0u;
  if (!g.last) return;
  if (fail)
  {
    st64(g.out, 0u);   // struck: whatever the buffer held, it does not begin with the magic
    *g.outSize = 0u;
    *g.status = kBlkCapacity;
    return;
  }
  const uint64_t totalSize = payload + payloadSize + kBlkPad;
  st64(g.out + kBlkHeader + 8ull * g.blockCount, payloadSize);
  st64(g.out, g.magic);
  st32(g.out + 8, 1u);
  st32(g.out + 12, 0u);
  st64(g.out + 16, g.inSize);
  st32(g.out + 24, g.blockSize);
  st32(g.out + 28, g.blockCount);
  st64(g.out + 32, payloadSize);
  st64(g.out + 40, totalSize);
  st64(g.out + 48, 0u);
  st64(g.out + 56, 0u);
  for (uint32_t k = 0; k < kBlkPad; k += 8u) st64(g.out + payload + payloadSize + k, 0u);
  *g.outSize = totalSize;
  *g.status = kBlkDone;
}

template <int UNUSED = 0>
__global__ __launch_bounds__(1024) void k_blk_scan(BlkScanArgs g)
{
  __shared__ uint64_t sSum[kBlkScanThreads];
  d_blk_scan(g, sSum);
}

// The stream of block b of a container of blockCount blocks and the bytes `cap` it may be read for.  The table entry is trusted in nothing: one that runs
// backwards or passes payloadSize gives a stream of no bytes, which a walk refuses without reading it.  (Every lane reads the same entry: wave-uniform.)
__device__ __forceinline__ const uint8_t *blk_stream(const uint8_t *container, uint32_t blockCount, uint64_t payloadSize, uint32_t b, uint32_t &cap)
{
  const uint8_t *table = container + kBlkHeader;
  const uint64_t e0 = ld64(table + 8ull * b), e1 = ld64(table + 8ull * b + 8u);
  const uint64_t o0 = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)e0) | (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(e0 >> 32)) << 32;
  const uint64_t o1 = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)e1) | (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(e1 >> 32)) << 32;
  const bool entry = o0 <= o1 && o1 <= payloadSize;
  const uint64_t len = entry ? o1 - o0 : 0u;
  cap = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;   // (S of the passes is capped by the ENTRY, never by the container)
  return table + 8ull * ((uint64_t)blockCount + 1u) + (entry ? o0 : 0u);
}

}   // namespace hsrle
