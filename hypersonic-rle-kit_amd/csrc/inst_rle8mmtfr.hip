// inst_rle8mmtfr.hip -- instantiates the kernels of the rle8_mmtf128 checkpoints and byte-range decode (hsrle_rle8mmtf_range.hip.h) and their launch sequences.
#include "hsrle_rle8mmtf_range.hip.h"
#include "hsrle_mmtf.h"

namespace hsrle {

hipError_t rle8mmtf_checkpoints_build_enqueue(const Rle8MmtfPlan &p, const uint8_t *dStream, uint32_t streamCap, const uint8_t *dIndex, uint32_t streamSize, uint32_t spacing,
                                              uint32_t entries, uint32_t checkpointRows, uint32_t count, uint8_t *dCheckpoints, uint64_t *dSize, uint32_t *dStatus, uint8_t *ws,
                                              hipStream_t st)
{
  hipError_t e = rle8mmtf_expand_indexed_enqueue(p, dStream, streamCap, dIndex, streamSize, spacing, entries, dStatus, ws, st);
  if (e != hipSuccess) return e;
  if (count != 0u && (e = mmtf128_decode_segments_enqueue(p.mmtf, ws + p.offRanks, ws + p.offMmtf, true, st)) != hipSuccess) return e;
  RmCkptArgs a;
  a.ranks = ws + p.offRanks;
  a.table = (uint32_t *)(ws + p.offMmtf + p.mmtf.offTable);
  a.ctrl = (const uint32_t *)ws;
  a.out = dCheckpoints;
  a.outSize = dSize;
  a.size = p.size; a.segRows = p.mmtf.R; a.checkpointRows = checkpointRows; a.count = count;
  const uint32_t wg = (count + 3u) / 4u;
  hipLaunchKernelGGL((k_rm_checkpoint_lists<0>), dim3(wg ? wg : 1u), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t rle8mmtf_decompress_range_enqueue(const RmRangePlan &p, const uint8_t *dStream, uint32_t streamCap, const uint8_t *dIndex, uint32_t streamSize, uint32_t spacing,
                                             uint32_t entries, const uint8_t *dCheckpoints, uint32_t checkpointRows, uint32_t count, uint8_t *dOut, uint64_t length,
                                             uint32_t *dStatus, uint8_t *ws, hipStream_t st)
{
  const uint32_t rows = p.r1 - p.c;
  RmRangeArgs a;
  a.d.stream = dStream;
  a.d.ranks = ws + p.offRanks;
  a.d.rec = (uint4 *)(ws + p.offRec);
  a.d.ctrl = (uint32_t *)ws;
  a.d.status = dStatus;
  a.d.streamCap = streamCap; a.d.size = p.size; a.d.rows = p.R; a.d.maxRec = p.maxRec;
  a.index = dIndex;
  a.ckpt = dCheckpoints;
  a.entries = entries;
  a.c = p.c; a.r1 = p.r1;
  a.start = p.c != 0u ? dCheckpoints + kRmCkptHeader + (uint64_t)(p.c / checkpointRows - 1u) * kRmCkptBytes : nullptr;
  for (uint32_t i = 0; i < 16u; i++)
  {
    a.wantIndex.w[i] = rm_index_header_word(i, p.size, streamSize, spacing, entries);
    a.wantCkpt.w[i] = rm_ckpt_header_word(i, p.size, streamSize, checkpointRows, count);
  }
  hipLaunchKernelGGL((k_rm_range_begin<0>), dim3(1), dim3(64), 0, st, a);
  hipLaunchKernelGGL((k_rm_walk_range<0>), dim3(p.stretches), dim3(64), 0, st, a);
  const uint32_t wg = (rows + 255u) / 256u;
  hipLaunchKernelGGL((k_rm_expand_range<0>), dim3(wg ? wg : 1u), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint8_t *bytes = ws + p.offRanks;   // (no row: every byte is a tail byte on an identity list, rank == symbol)
  if (rows != 0u)
  {
    if ((e = mmtf128_decode_segments_enqueue(p.mmtf, ws + p.offRanks, ws + p.offMmtf, false, st)) != hipSuccess) return e;
    MmtfArgs m;
    m.in = ws + p.offRanks; m.out = ws + p.offStage;
    m.table = (uint32_t *)(ws + p.offMmtf + p.mmtf.offTable);
    m.counts = (uint32_t *)(ws + p.offMmtf + p.mmtf.offCounts);
    m.size = p.mmtf.size; m.rows = p.mmtf.rows; m.R = p.mmtf.R; m.S = p.mmtf.S;
    if (m.S > 1u) hipLaunchKernelGGL((k_rm_range_scan<0>), dim3(16), dim3(64), 0, st, m, a.start);
    hipLaunchKernelGGL((k_rm_range_rows<0>), dim3((uint32_t)(((uint64_t)m.S * 16u + 63u) / 64u)), dim3(64), 0, st, m, a.start);
    bytes = ws + p.offStage;
  }
  const uint64_t pieces = (length + 4095u) / 4096u;
  hipLaunchKernelGGL((k_rm_range_copy<0>), dim3((uint32_t)(pieces > 4096u ? 4096u : pieces)), dim3(256), 0, st, bytes + p.skip, dOut, length, (const uint32_t *)ws);
  return hipGetLastError();
}

}   // namespace hsrle
