// inst_rle8mmtf.hip -- instantiates the rle8_mmtf128 kernels (hsrle_rle8mmtf.hip.h) and their launch sequences around the mmtf128 plan.
#include "hsrle_rle8mmtf.hip.h"
#include "hsrle_mmtf.h"

namespace hsrle {

hipError_t rle8mmtf_compress_enqueue(const Rle8MmtfPlan &p, const uint8_t *dIn, uint8_t *dOut, uint32_t outCap, uint32_t *dOutSize, uint32_t *dStatus, uint8_t *ws, hipStream_t st)
{
  RmEncArgs a;
  a.ranks = ws + p.offRanks;
  a.out = dOut;
  a.sum = (uint4 *)(ws + p.offA);
  a.res = (uint4 *)(ws + p.offB);
  a.ctrl = (uint32_t *)ws;
  a.outSize = dOutSize;
  a.status = dStatus;
  a.size = p.size; a.rows = p.rows; a.SP = p.SP; a.spans = p.spans; a.outCap = outCap;
  const hipError_t e = mmtf_enqueue(p.mmtf, false, dIn, ws + p.offRanks, ws + p.offMmtf, st);
  if (e != hipSuccess) return e;
  const uint32_t wg = (p.spans + 3u) / 4u;
  if (wg) hipLaunchKernelGGL((k_rm_classify<0>), dim3(wg), dim3(256), 0, st, a);
  hipLaunchKernelGGL((k_rm_scan<0>), dim3(1), dim3(kRmScanThreads), 0, st, a);
  if (wg) hipLaunchKernelGGL((k_rm_emit<0>), dim3(wg), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t rle8mmtf_decompress_enqueue(const Rle8MmtfPlan &p, const uint8_t *dStream, uint32_t streamCap, uint8_t *dOut, uint32_t *dStatus, uint8_t *ws, hipStream_t st)
{
  RmDecArgs a;
  a.stream = dStream;
  a.ranks = ws + p.offRanks;
  a.rec = (uint4 *)(ws + p.offA);
  a.ctrl = (uint32_t *)ws;
  a.status = dStatus;
  a.streamCap = streamCap; a.size = p.size; a.rows = p.rows; a.maxRec = p.maxRec;
  hipLaunchKernelGGL((k_rm_walk<0>), dim3(1), dim3(64), 0, st, a);
  const uint32_t wg = (p.rows + 255u) / 256u;
  hipLaunchKernelGGL((k_rm_expand<0>), dim3(wg ? wg : 1u), dim3(256), 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return mmtf_enqueue(p.mmtf, true, ws + p.offRanks, dOut, ws + p.offMmtf, st);
}

}   // namespace hsrle
