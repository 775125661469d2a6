// inst_rle8sh.hip -- instantiates the rle8_sh kernels (hsrle_rle8sh.hip.h) and their launch sequences.
#include "hsrle_rle8sh.hip.h"
#include "hsrle_rle8sh.h"

namespace hsrle {

hipError_t rle8sh_compress_enqueue(const ShEncPlan &p, const uint8_t *dIn, uint8_t *dOut, uint32_t outCap, uint32_t *dOutSize, uint32_t *dStatus, uint8_t *ws, hipStream_t st)
{
  ShEncArgs a;
  a.in = dIn;
  a.out = dOut;
  a.items = (uint4 *)(ws + p.offItems);
  a.er = (uint4 *)(ws + p.offEr);
  a.bits = (uint32_t *)(ws + p.offBits);
  a.ctrl = (uint32_t *)ws;
  a.outSize = dOutSize;
  a.status = dStatus;
  a.size = p.size; a.maxItems = p.maxItems; a.maxEr = p.maxEr; a.bitWords = p.bitWords; a.outCap = outCap;
  const uint32_t bitGrid = (p.bitWords + 255u) / 256u;
  hipLaunchKernelGGL((k_she_decide<0>), dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL((k_she_code<0>), dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL((k_she_zero<0>), dim3(bitGrid), dim3(256), 0, st, a);
  hipLaunchKernelGGL((k_she_emit<0>), dim3((p.maxEr + 255u) / 256u), dim3(256), 0, st, a);
  hipLaunchKernelGGL((k_she_raw<0>), dim3((p.size + 4095u) / 4096u), dim3(256), 0, st, a);
  hipLaunchKernelGGL((k_she_place<0>), dim3(bitGrid), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t rle8sh_decompress_enqueue(const ShPlan &p, const uint8_t *dStream, uint32_t streamCap, uint8_t *dOut, uint32_t *dStatus, uint8_t *ws, hipStream_t st)
{
  ShDecArgs a;
  a.stream = dStream;
  a.out = dOut;
  a.rec = (uint4 *)(ws + p.offRec);
  a.st = (uint2 *)(ws + p.offState);
  a.ctrl = (uint32_t *)ws;
  a.status = dStatus;
  a.streamCap = streamCap; a.size = p.size; a.maxRec = p.maxRec; a.cap = p.cap; a.win = p.win; a.force = p.force;
  const uint32_t recGrid = (p.maxRec + 255u) / 256u;
  hipLaunchKernelGGL((k_sh_walk<0>), dim3(1), dim3(64), 0, st, a);
  if (!p.force) hipLaunchKernelGGL((k_sh_summary<0>), dim3(recGrid), dim3(256), 0, st, a);
  hipLaunchKernelGGL((k_sh_scan<0>), dim3(1), dim3(kShScanThreads), 0, st, a);
  hipLaunchKernelGGL((k_sh_expand_blocks<0>), dim3((p.size + 4095u) / 4096u), dim3(256), 0, st, a);
  if (!p.force) hipLaunchKernelGGL((k_sh_expand_sym<0>), dim3(recGrid), dim3(256), 0, st, a);
  // the fallback, gated on the device by ctrl[2]: the serial symbol pass and the expansion from its states
  hipLaunchKernelGGL((k_sh_state<0>), dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL((k_sh_expand_sym<1>), dim3(recGrid), dim3(256), 0, st, a);
  return hipGetLastError();
}

}   // namespace hsrle
