// inst_rle8shb.hip -- instantiates the kernels of the blocked rle8_sh (hsrle_rle8shb.hip.h) and their launch sequences: a loop over groups of blocks.
#include "hsrle_rle8shb.hip.h"
#include "hsrle_rle8sh.h"

namespace hsrle {

hipError_t rle8shb_compress_enqueue(const ShbPlan &p, const uint8_t *dIn, uint8_t *dOut, uint64_t outCap, uint64_t *dOutSize, uint32_t *dStatus, uint8_t *ws, hipStream_t st)
{
  ShbEncArgs g;
  g.in = dIn;
  g.out = dOut;
  g.slots = ws + 256;
  g.run = (uint32_t *)ws;
  g.outSize = dOutSize;
  g.status = dStatus;
  g.inSize = p.size; g.outCap = outCap; g.slotStride = p.enc.total; g.offItems = p.enc.offItems; g.offEr = p.enc.offEr; g.offBits = p.enc.offBits;
  g.blockSize = p.blockSize; g.blockCount = p.blockCount; g.maxItems = p.enc.maxItems; g.maxEr = p.enc.maxEr; g.bitWords = p.enc.bitWords;
  hipLaunchKernelGGL((k_blk_begin<0>), dim3(1), dim3(64), 0, st, g.run, 3u);
  for (uint32_t first = 0u; first < p.blockCount; first += p.inFlight)
  {
    g.first = first;
    g.count = p.blockCount - first < p.inFlight ? p.blockCount - first : p.inFlight;
    g.last = first + g.count == p.blockCount ? 1u : 0u;
    hipLaunchKernelGGL((k_shb_decide_code<0>), dim3(g.count), dim3(64), 0, st, g);
    hipLaunchKernelGGL((k_blk_scan<0>), dim3(1), dim3(kBlkScanThreads), 0, st, shb_scan_args(g));
    hipLaunchKernelGGL((k_shb_write<0>), dim3(g.count), dim3(64), 0, st, g);
  }
  return hipGetLastError();
}

hipError_t rle8shb_decompress_enqueue(const ShbPlan &p, const uint8_t *dContainer, uint64_t payloadSize, uint32_t firstBlock, uint32_t blockCount, uint8_t *dOut,
                                      uint32_t *dStatus, uint8_t *ws, hipStream_t st)
{
  ShbDecArgs g;
  g.container = dContainer;
  g.out = dOut;
  g.slots = ws + 256;
  g.status = dStatus;
  g.size = p.size; g.payloadSize = payloadSize; g.slotStride = p.dec.total; g.offRec = p.dec.offRec; g.offState = p.dec.offState;
  g.blockSize = p.blockSize; g.blockCount = p.blockCount; g.maxRec = p.dec.maxRec; g.cap = p.dec.cap; g.win = p.dec.win;
  hipLaunchKernelGGL((k_blk_begin<0>), dim3(1), dim3(64), 0, st, dStatus, 1u);
  for (uint32_t done = 0u; done < blockCount; done += p.inFlight)
  {
    g.first = firstBlock + done;
    g.count = blockCount - done < p.inFlight ? blockCount - done : p.inFlight;
    hipLaunchKernelGGL((k_shb_decode<0>), dim3(g.count), dim3(64), 0, st, g);
  }
  return hipGetLastError();
}

}   // namespace hsrle
