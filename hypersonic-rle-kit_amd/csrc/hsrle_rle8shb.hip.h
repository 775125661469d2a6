// hsrle_rle8shb.hip.h -- the BLOCKED form of rle8_sh (include/hsrle.h section 5, "rle8_sh block container"): the input is cut into blocks and every
// block is a complete rle8_sh stream of its own, so the passes that are one wave or one lane for a whole stream (hsrle_rle8sh.hip.h: decide, code,
// walk, state) run for thousands of streams at once.  Nothing of the codec is restated here: a workgroup of ONE wave finds its block, makes the
// ShEncArgs / ShDecArgs of that block -- its slice of the input, of the payload and of the workspace -- and calls the passes of hsrle_rle8sh.hip.h.
//
// Container: 64 header bytes, u64 offset[blockCount + 1] (relative to the payload), the block streams back to back at ANY byte address, 32 zero
// bytes.  Neighbouring streams are written at the same time, so no pass may store beyond its own stream or read-modify-write a word of it: the passes
// store the body byte by byte or as whole words INSIDE a record, 16 bytes only inside a raw COPY, and the bit stream is placed byte by byte.
//
// Blocks go through in GROUPS of `count` (the host loops and only enqueues); a block of the group owns slot `blockIdx.x` of the workspace.
//   encode  k_blk_begin          the running payload size and the does-not-fit word: zero
//           k_shb_decide_code    per block: decide, then the symbol state and the sizes (lane 0)
//           k_blk_scan           ONE workgroup (hsrle_blockscan.hip.h): exclusive scan of the group's stream sizes onto the running payload size; the offset
//                                table; whether the group still fits; behind the last group the header, the pad, the size word and the status (or the
//                                struck magic)
//           k_shb_write          per block: zero, emit, raw, place -- straight to the stream's final address
//   decode  k_blk_begin          the status word: DONE
//           k_shb_decode         per block: its table entry (trusted in nothing), walk -- every verdict, before anything is written --, the serial symbol
//                                state (lane 0: a block has few records), the two expansions
// Inside a kernel the passes of a block meet through global memory of the SAME workgroup: blk_pass_edge stands between them.
#pragma once

#include "hsrle_rle8sh.hip.h"
#include "hsrle_blockscan.hip.h"

namespace hsrle {

constexpr uint32_t kShbHeader = kBlkHeader;
// words of a slot's control block behind those of the passes ([0..4]): the size and status words the single-stream passes write, the stream's place
constexpr uint32_t kShbSize = 8u, kShbStatus = 9u, kShbAtLo = kBlkAtLo, kShbAtHi = kBlkAtHi;

struct ShbEncArgs
{
  const uint8_t *in;
  uint8_t *out;          // the container
  uint8_t *slots;        // slot 0; a slot is the workspace of a single stream of blockSize bytes
  uint32_t *run;         // [0], [1] payload bytes of the groups before this one, [2] 1: the container does not fit
  uint64_t *outSize;
  uint32_t *status;
  uint64_t inSize, outCap, slotStride, offItems, offEr, offBits;
  uint32_t blockSize, blockCount, first, count, maxItems, maxEr, bitWords, last;   // blocks [first, first + count) of blockCount; last: the last group
};

struct ShbDecArgs
{
  const uint8_t *container;
  uint8_t *out;
  uint8_t *slots;
  uint32_t *status;
  uint64_t size, payloadSize, slotStride, offRec, offState;
  uint32_t blockSize, blockCount, first, count, maxRec, cap, win;   // blocks [first, first + count) of the container's blockCount
};

__device__ __forceinline__ ShEncArgs shb_enc_args(const ShbEncArgs &g, uint32_t j)
{
  uint8_t *ws = g.slots + (uint64_t)j * g.slotStride;
  const uint64_t at = (uint64_t)(g.first + j) * g.blockSize, left = g.inSize - at;
  ShEncArgs a;
  a.in = g.in + at;
  a.out = nullptr;
  a.items = (uint4 *)(ws + g.offItems);
  a.er = (uint4 *)(ws + g.offEr);
  a.bits = (uint32_t *)(ws + g.offBits);
  a.ctrl = (uint32_t *)ws;
  a.outSize = a.ctrl + kShbSize;
  a.status = a.ctrl + kShbStatus;
  a.size = left < g.blockSize ? (uint32_t)left : g.blockSize;
  a.maxItems = g.maxItems; a.maxEr = g.maxEr; a.bitWords = g.bitWords;
  a.outCap = 0xFFFFFFFFu;   // (whether the stream fits is the scan's question)
  return a;
}

template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_shb_decide_code(ShbEncArgs g)
{
  const ShEncArgs a = shb_enc_args(g, blockIdx.x);
  d_she_decide(a);
  blk_pass_edge();
  d_she_code(a);
}

inline BlkScanArgs shb_scan_args(const ShbEncArgs &g)
{
  BlkScanArgs b;
  b.out = g.out; b.slots = g.slots; b.run = g.run; b.outSize = g.outSize; b.status = g.status;
  b.inSize = g.inSize; b.outCap = g.outCap; b.slotStride = g.slotStride;
  b.magic = 0x424853454C525348ull;   // "HSRLESHB"
  b.blockSize = g.blockSize; b.blockCount = g.blockCount; b.first = g.first; b.count = g.count; b.last = g.last;
  return b;
}

template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_shb_write(ShbEncArgs g)
{
  ShEncArgs a = shb_enc_args(g, blockIdx.x);
  if (a.ctrl[0] != 0u) return;
  const uint64_t at = (uint64_t)a.ctrl[kShbAtLo] | (uint64_t)a.ctrl[kShbAtHi] << 32;
  a.out = g.out + kShbHeader + 8ull * ((uint64_t)g.blockCount + 1u) + at;
  const uint32_t lane = threadIdx.x, bitWords = (a.ctrl[4] + 3u) / 4u, records = a.ctrl[2], chunks = (a.size + 15u) / 16u;
  for (uint32_t i = lane; i < bitWords; i += 64u) d_she_zero(a, i);
  blk_pass_edge();   // (the token bits are ORed into the zeroed words)
  for (uint32_t i = lane; i < records; i += 64u) d_she_emit(a, i);
  for (uint32_t i = lane; i < chunks; i += 64u) d_she_raw(a, i);
  blk_pass_edge();
  for (uint32_t i = lane; i < bitWords; i += 64u) d_she_place(a, i);   // (the terminator's bits: at least one word, so lane 0 writes the header)
}

template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_shb_decode(ShbDecArgs g)
{
  uint8_t *ws = g.slots + (uint64_t)blockIdx.x * g.slotStride;
  const uint32_t b = g.first + blockIdx.x, lane = threadIdx.x;
  const uint64_t at = (uint64_t)b * g.blockSize, left = g.size - at;
  ShDecArgs a;
  a.stream = blk_stream(g.container, g.blockCount, g.payloadSize, b, a.streamCap);
  a.out = g.out + at;
  a.rec = (uint4 *)(ws + g.offRec);
  a.st = (uint2 *)(ws + g.offState);
  a.ctrl = (uint32_t *)ws;
  a.status = a.ctrl + kShbStatus;
  a.size = left < g.blockSize ? (uint32_t)left : g.blockSize;
  a.maxRec = g.maxRec; a.cap = g.cap; a.win = g.win; a.force = 1u;
  d_sh_walk(a);
  if (lane == 0u)
  {
    a.ctrl[2] = 1u;   // the serial symbol pass is this decoder's only one
    if (a.ctrl[0] != kShDone) atomicOr(g.status, kShMalformed);
  }
  blk_pass_edge();
  if (a.ctrl[0] != kShDone) return;   // a malformed block: none of its bytes is written
  d_sh_state(a);
  blk_pass_edge();
  const uint32_t chunks = (a.size + 15u) / 16u, records = a.ctrl[1];
  for (uint32_t i = lane; i < chunks; i += 64u) d_sh_expand_blocks(a, i);
  for (uint32_t i = lane; i < records; i += 64u) d_sh_expand_sym<1>(a, i);
}

}   // namespace hsrle
