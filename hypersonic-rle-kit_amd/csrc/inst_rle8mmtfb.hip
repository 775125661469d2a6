// inst_rle8mmtfb.hip -- instantiates the kernels of the blocked rle8_mmtf128 (hsrle_rle8mmtfb.hip.h) and their launch sequences: a loop over groups of blocks.
#include "hsrle_rle8mmtfb.hip.h"
#include "hsrle_mmtf.h"

namespace hsrle {

hipError_t rle8mmtfb_compress_enqueue(const MfbPlan &p, const uint8_t *dIn, uint8_t *dOut, uint64_t outCap, uint64_t *dOutSize, uint32_t *dStatus, uint8_t *ws, hipStream_t st)
{
  MfbEncArgs g;
  g.in = dIn;
  g.out = dOut;
  g.slots = ws + 256;
  g.inSize = p.size; g.slotStride = p.encSlot; g.offRanks = p.offRanks; g.offSum = p.offA; g.offRes = p.offB;
  g.blockSize = p.blockSize; g.blockCount = p.blockCount; g.SP = p.SP;
  MfbRowsArgs r;
  r.data = const_cast<uint8_t *>(dIn);   // (the encode direction only reads it)
  r.slots = g.slots;
  r.size = p.size; r.slotStride = p.encSlot; r.offRanks = p.offRanks;
  r.blockSize = p.blockSize;
  BlkScanArgs s;
  s.out = dOut; s.slots = g.slots; s.run = (uint32_t *)ws; s.outSize = dOutSize; s.status = dStatus;
  s.inSize = p.size; s.outCap = outCap; s.slotStride = p.encSlot;
  s.magic = 0x42464D454C525348ull;   // "HSRLEMFB"
  s.blockSize = p.blockSize; s.blockCount = p.blockCount;
  hipLaunchKernelGGL((k_blk_begin<0>), dim3(1), dim3(64), 0, st, s.run, 3u);
  for (uint32_t first = 0u; first < p.blockCount; first += p.inFlight)
  {
    const uint32_t count = p.blockCount - first < p.inFlight ? p.blockCount - first : p.inFlight;
    g.first = r.first = s.first = first;
    g.count = r.count = s.count = count;
    s.last = first + count == p.blockCount ? 1u : 0u;
    hipLaunchKernelGGL((k_mfb_rows<false>), dim3((count + 3u) / 4u), dim3(64), 0, st, r);
    hipLaunchKernelGGL((k_mfb_place<0>), dim3(count), dim3(64), 0, st, g);
    hipLaunchKernelGGL((k_blk_scan<0>), dim3(1), dim3(kBlkScanThreads), 0, st, s);
    hipLaunchKernelGGL((k_mfb_write<0>), dim3(count), dim3(64), 0, st, g);
  }
  return hipGetLastError();
}

hipError_t rle8mmtfb_decompress_enqueue(const MfbPlan &p, const uint8_t *dContainer, uint64_t payloadSize, uint32_t firstBlock, uint32_t blockCount, uint8_t *dOut,
                                        uint32_t *dStatus, uint8_t *ws, hipStream_t st)
{
  MfbDecArgs g;
  g.container = dContainer;
  g.out = dOut;
  g.slots = ws + 256;
  g.status = dStatus;
  g.size = p.size; g.payloadSize = payloadSize; g.slotStride = p.decSlot; g.offRanks = p.offRanks; g.offRec = p.offA;
  g.blockSize = p.blockSize; g.blockCount = p.blockCount; g.maxRec = p.maxRec;
  MfbRowsArgs r;
  r.data = dOut;
  r.slots = g.slots;
  r.size = p.size; r.slotStride = p.decSlot; r.offRanks = p.offRanks;
  r.blockSize = p.blockSize;
  hipLaunchKernelGGL((k_blk_begin<0>), dim3(1), dim3(64), 0, st, dStatus, 1u);
  for (uint32_t done = 0u; done < blockCount; done += p.inFlight)
  {
    g.first = r.first = firstBlock + done;
    g.count = r.count = blockCount - done < p.inFlight ? blockCount - done : p.inFlight;
    hipLaunchKernelGGL((k_mfb_walk_expand<0>), dim3(g.count), dim3(64), 0, st, g);
    hipLaunchKernelGGL((k_mfb_rows<true>), dim3((g.count + 3u) / 4u), dim3(64), 0, st, r);
  }
  return hipGetLastError();
}

}   // namespace hsrle
