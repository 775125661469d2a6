// inst_rle8mmtfi.hip -- instantiates the kernels of the rle8_mmtf128 entry index (hsrle_rle8mmtf_index.hip.h) and their launch sequences.
#include "hsrle_rle8mmtf_index.hip.h"
#include "hsrle_mmtf.h"

namespace hsrle {

// behind rle8mmtf_compress_enqueue of the same plan on the same stream: the tables of its workspace are read as k_rm_emit left them
hipError_t rle8mmtf_index_emit_enqueue(const Rle8MmtfPlan &p, uint8_t *dOut, uint32_t *dOutSize, uint8_t *ws, uint32_t spacing, uint8_t *dIndex, uint64_t *dIndexSize, hipStream_t st)
{
  RmIdxEncArgs a;
  a.e.ranks = ws + p.offRanks;
  a.e.out = dOut;
  a.e.sum = (uint4 *)(ws + p.offA);
  a.e.res = (uint4 *)(ws + p.offB);
  a.e.ctrl = (uint32_t *)ws;
  a.e.outSize = dOutSize;
  a.e.status = nullptr;
  a.e.size = p.size; a.e.rows = p.rows; a.e.SP = p.SP; a.e.spans = p.spans; a.e.outCap = 0u;
  a.index = dIndex;
  a.indexSize = dIndexSize;
  a.spacing = spacing;
  hipLaunchKernelGGL((k_rm_index_count<0>), dim3(1), dim3(kRmScanThreads), 0, st, a);
  const uint32_t wg = (p.spans + 3u) / 4u;
  if (wg) hipLaunchKernelGGL((k_rm_index_emit<0>), dim3(wg), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t rle8mmtf_index_build_enqueue(const uint8_t *dStream, uint32_t streamCap, uint32_t size, uint32_t spacing, uint8_t *dIndex, uint64_t *dIndexSize, uint32_t *dStatus,
                                        hipStream_t st)
{
  RmIdxBuildArgs a;
  a.d.stream = dStream;
  a.d.ranks = nullptr;
  a.d.rec = nullptr;
  a.d.ctrl = nullptr;
  a.d.status = dStatus;
  a.d.streamCap = streamCap; a.d.size = size; a.d.rows = size / 16u; a.d.maxRec = 0xFFFFFFFFu;
  a.index = dIndex;
  a.indexSize = dIndexSize;
  a.spacing = spacing;
  hipLaunchKernelGGL((k_rm_index_build<0>), dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t rle8mmtf_expand_indexed_enqueue(const Rle8MmtfPlan &p, const uint8_t *dStream, uint32_t streamCap, const uint8_t *dIndex, uint32_t streamSize, uint32_t spacing,
                                           uint32_t entries, uint32_t *dStatus, uint8_t *ws, hipStream_t st)
{
  RmIdxDecArgs a;
  a.d.stream = dStream;
  a.d.ranks = ws + p.offRanks;
  a.d.rec = (uint4 *)(ws + p.offA);
  a.d.ctrl = (uint32_t *)ws;
  a.d.status = dStatus;
  a.d.streamCap = streamCap; a.d.size = p.size; a.d.rows = p.rows; a.d.maxRec = p.maxRec;
  a.index = dIndex;
  a.entries = entries;
  for (uint32_t i = 0; i < 16u; i++) a.want.w[i] = rm_index_header_word(i, p.size, streamSize, spacing, entries);
  hipLaunchKernelGGL((k_rm_index_begin<0>), dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL((k_rm_walk_indexed<0>), dim3(entries + 1u), dim3(64), 0, st, a);
  const uint32_t wg = (p.rows + 255u) / 256u;
  hipLaunchKernelGGL((k_rm_expand_indexed<0>), dim3(wg ? wg : 1u), dim3(256), 0, st, a.d);
  return hipGetLastError();
}

hipError_t rle8mmtf_decompress_indexed_enqueue(const Rle8MmtfPlan &p, const uint8_t *dStream, uint32_t streamCap, const uint8_t *dIndex, uint32_t streamSize, uint32_t spacing,
                                               uint32_t entries, uint8_t *dOut, uint32_t *dStatus, uint8_t *ws, hipStream_t st)
{
  const hipError_t e = rle8mmtf_expand_indexed_enqueue(p, dStream, streamCap, dIndex, streamSize, spacing, entries, dStatus, ws, st);
  if (e != hipSuccess) return e;
  return mmtf_enqueue(p.mmtf, true, ws + p.offRanks, dOut, ws + p.offMmtf, st);
}

}   // namespace hsrle
