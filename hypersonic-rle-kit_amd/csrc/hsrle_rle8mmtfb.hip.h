// hsrle_rle8mmtfb.hip.h -- the BLOCKED form of rle8_mmtf128 (include/hsrle.h section 5, "rle8_mmtf128 block container"): the input is cut into blocks and
// every block is a complete rle8_mmtf128 stream of its own, its move-to-front lists the identity at its first byte.  So the three serial parts of the
// single stream go: the transform of a block needs no state table, no pass A and no scan (a lane per block and column runs what is pass C there), the
// span scan of a block is the work of one wave, and every block's header chain is walked by a wave of its own.  Nothing of the codec is restated here:
// the kernels find their block, make the RmEncArgs / RmDecArgs of that block -- its slice of the input, of the payload and of the workspace -- and call
// the passes of hsrle_rle8mmtf.hip.h and the row loop of hsrle_mmtf.hip.h.
//
// Container and groups: hsrle_blockscan.hip.h.  Neighbouring streams are written at the same time at any byte address: d_rm_emit and d_rm_close store
// whole bytes, words and vectors INSIDE the packet or header they belong to, so no store reaches beyond its own stream and no word is read-modify-
// written.  A block's passes read rank rows from the block's OWN rank buffer only (the other rows of a 2 / 3 / 4 bit group lie below the block's last row).
//   encode  k_blk_begin          the running payload size and the does-not-fit word: zero
//           k_mfb_rows<false>    a lane per (block, column), four blocks per wave: the block's bytes -> its rank buffer, from identity lists
//           k_mfb_place          a wave per block: classify its spans, then close and place its packets (the span scan, inside the wave); the stream's size
//           k_blk_scan           ONE workgroup: the streams' places, the offset table, the fit verdict, behind the last group header, pad and size word
//           k_mfb_write          a wave per block: emit, the chain's end, the tail ranks, the stream header -- straight to the stream's final address
//   decode  k_blk_begin          the status word: DONE
//           k_mfb_walk_expand    a wave per block: its table entry (trusted in nothing), the walk -- every verdict, before anything is written --, the
//                                expansion into the block's rank buffer
//           k_mfb_rows<true>     a lane per (block, column): the inverse transform from identity lists into the output, only for a block whose verdict is DONE
#pragma once

#include "hsrle_mmtf.hip.h"
#include "hsrle_rle8mmtf.hip.h"
#include "hsrle_blockscan.hip.h"

namespace hsrle {

// words of a slot's control block: [0 .. 2] the passes' own (hsrle_rle8mmtf.hip.h), [3], [10], [11] the group scan's (hsrle_blockscan.hip.h), and
constexpr uint32_t kMfbAt = 5u, kMfbEnd = 6u;           // encode: the offset behind the last packet, the bytes of the chain's end
constexpr uint32_t kMfbSize = 8u, kMfbStatus = 9u;      // the size and status words that the single-stream passes write

struct MfbEncArgs
{
  const uint8_t *in;
  uint8_t *out;          // the container
  uint8_t *slots;        // slot 0: control words, the block's rank buffer, its span summaries and span results
  uint64_t inSize, slotStride, offRanks, offSum, offRes;
  uint32_t blockSize, blockCount, first, count, SP;   // blocks [first, first + count) of blockCount
};

struct MfbDecArgs
{
  const uint8_t *container;
  uint8_t *out;
  uint8_t *slots;        // slot 0: control words, the block's rank buffer, its packet records
  uint32_t *status;
  uint64_t size, payloadSize, slotStride, offRanks, offRec;
  uint32_t blockSize, blockCount, first, count, maxRec;   // blocks [first, first + count) of the container's blockCount
};

// the transform of the group's blocks, either direction: `data` is the whole input (encode) or the whole output (decode)
struct MfbRowsArgs
{
  uint8_t *data;
  uint8_t *slots;
  uint64_t size, slotStride, offRanks;
  uint32_t blockSize, first, count;
};

__device__ __forceinline__ uint32_t mfb_block_bytes(uint64_t size, uint32_t blockSize, uint32_t b)
{
  const uint64_t left = size - (uint64_t)b * blockSize;
  return left < blockSize ? (uint32_t)left : blockSize;
}

template <bool DEC>
__global__ __launch_bounds__(64) void k_mfb_rows(MfbRowsArgs g)
{
  __shared__ uint32_t sList[kMmtfGroupDwords];
  __shared__ __attribute__((aligned(16))) uint8_t sTile[1024];
  const uint32_t lane = threadIdx.x, j = blockIdx.x * 4u + lane / 16u, col = lane % 16u;
  bool valid = j < g.count;
  uint8_t *ranks = g.slots, *bytes = g.data;
  uint32_t size = 0u;
  if (valid)
  {
    uint8_t *ws = g.slots + (uint64_t)j * g.slotStride;
    if (DEC && ((const uint32_t *)ws)[0] != kRmDone) valid = false;   // a malformed block: none of its bytes is written
    else
    {
      ranks = ws + g.offRanks;
      bytes = g.data + (uint64_t)(g.first + j) * g.blockSize;
      size = mfb_block_bytes(g.size, g.blockSize, g.first + j);
    }
  }
  const uint8_t *src = DEC ? ranks : bytes;
  uint8_t *dst = DEC ? bytes : ranks;
  const uint32_t rows = size / 16u;
  MmtfList L;
  L.lds = sList + lane;
  L.identity();
  uint32_t K = 0;
  d_mmtf_rows<16, DEC, true>(L, K, src, dst, rows, (g.blockSize / 16u + 15u) / 16u, col, sTile + (lane / 16u) * 256u);
  const uint32_t i = rows * 16u + col;   // the tail: byte `col` behind the last row, column `col`'s list as it stands
  if (valid && i < size) dst[i] = (uint8_t)(DEC ? L.at(src[i]) : L.rank_of(src[i]));
}

__device__ __forceinline__ RmEncArgs mfb_enc_args(const MfbEncArgs &g, uint32_t j)
{
  uint8_t *ws = g.slots + (uint64_t)j * g.slotStride;
  RmEncArgs a;
  a.ranks = ws + g.offRanks;
  a.out = nullptr;
  a.sum = (uint4 *)(ws + g.offSum);
  a.res = (uint4 *)(ws + g.offRes);
  a.ctrl = (uint32_t *)ws;
  a.outSize = a.ctrl + kMfbSize;
  a.status = a.ctrl + kMfbStatus;
  a.size = mfb_block_bytes(g.inSize, g.blockSize, g.first + j);
  a.rows = a.size / 16u;
  a.SP = g.SP;
  a.spans = (a.rows + g.SP - 1u) / g.SP;
  a.outCap = 0xFFFFFFFFu;   // (whether the stream fits is the group scan's question)
  return a;
}

template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_mfb_place(MfbEncArgs g)
{
  __shared__ uint32_t sA[64], sB[64];
  __shared__ uint32_t sTotal;
  const RmEncArgs a = mfb_enc_args(g, blockIdx.x);
  const uint32_t lane = threadIdx.x;
  for (uint32_t span = 0u; span < a.spans; span++) d_rm_classify(a, span, lane);
  blk_pass_edge();
  const uint32_t at = d_rm_scan<64u>(a, lane, sA, sB, &sTotal);
  if (lane != 0u) return;
  const uint32_t end = rm_chain_end(a);
  a.ctrl[kBlkFail] = 0u;
  a.ctrl[kBlkStreamSize] = at + end + (a.size - a.rows * 16u);
  a.ctrl[kMfbAt] = at;
  a.ctrl[kMfbEnd] = end;
}

template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_mfb_write(MfbEncArgs g)
{
  RmEncArgs a = mfb_enc_args(g, blockIdx.x);
  if (a.ctrl[kBlkFail] != 0u) return;
  const uint64_t at = (uint64_t)a.ctrl[kBlkAtLo] | (uint64_t)a.ctrl[kBlkAtHi] << 32;
  a.out = g.out + kBlkHeader + 8ull * ((uint64_t)g.blockCount + 1u) + at;
  const uint32_t lane = threadIdx.x;
  for (uint32_t span = 0u; span < a.spans; span++) d_rm_emit(a, span, lane);
  if (lane == 0u) d_rm_close(a, a.ctrl[kMfbAt], a.ctrl[kMfbEnd]);
}

template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_mfb_walk_expand(MfbDecArgs g)
{
  __shared__ __attribute__((aligned(16))) uint8_t sWin[kRmWalkWindow];
  uint8_t *ws = g.slots + (uint64_t)blockIdx.x * g.slotStride;
  const uint32_t b = g.first + blockIdx.x, lane = threadIdx.x;
  RmDecArgs a;
  a.stream = blk_stream(g.container, g.blockCount, g.payloadSize, b, a.streamCap);
  a.ranks = ws + g.offRanks;
  a.rec = (uint4 *)(ws + g.offRec);
  a.ctrl = (uint32_t *)ws;
  a.status = a.ctrl + kMfbStatus;
  a.size = mfb_block_bytes(g.size, g.blockSize, b);
  a.rows = a.size / 16u;
  a.maxRec = g.maxRec;
  d_rm_walk(a, sWin, lane);
  if (lane == 0u && a.ctrl[0] != kRmDone) atomicOr(g.status, kRmMalformed);
  blk_pass_edge();
  if (a.ctrl[0] != kRmDone) return;   // a malformed block: nothing is expanded, and k_mfb_rows<true> leaves its bytes alone
  for (uint32_t row0 = 0u; row0 < a.rows; row0 += 64u) d_rm_expand(a, row0, lane);
  d_rm_expand_tail(a, lane);
}

}   // namespace hsrle
