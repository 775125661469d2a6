// inst_mmtf.hip -- instantiates the mmtf / bitmmtf kernels (hsrle_mmtf.hip.h) and their launch sequence.
#include "hsrle_mmtf.hip.h"
#include "hsrle_mmtf.h"

namespace hsrle {

template <int W, bool DEC>
static hipError_t mmtf_rows_enqueue(const MmtfArgs &a, hipStream_t st)
{
  if (a.S > 1u)
  {
    const uint64_t lanesA = (uint64_t)(a.S - 1u) * W;
    hipLaunchKernelGGL((k_mmtf_rows<W, DEC, false>), dim3((uint32_t)((lanesA + 63u) / 64u)), dim3(64), 0, st, a);
    if (DEC) hipLaunchKernelGGL((k_mmtf_scan_dec<W>), dim3(W), dim3(64), 0, st, a);
    else hipLaunchKernelGGL((k_mmtf_scan_enc<W>), dim3(W), dim3(64), 0, st, a);
  }
  const uint64_t lanesC = (uint64_t)a.S * W;
  hipLaunchKernelGGL((k_mmtf_rows<W, DEC, true>), dim3((uint32_t)((lanesC + 63u) / 64u)), dim3(64), 0, st, a);
  return hipGetLastError();
}

template <int E>
static hipError_t bitmmtf_enqueue(const MmtfPlan &p, bool decode, const uint8_t *in, uint8_t *out, uint32_t *vals, hipStream_t st)
{
  const uint32_t m = p.size & ~(uint32_t)(E - 1);
  if (!decode)
  {
    const uint64_t wg = (((uint64_t)m + 15u) / 16u + 255u) / 256u;
    hipLaunchKernelGGL((k_bitmmtf_enc<E>), dim3((uint32_t)(wg < 1u ? 1u : (wg > 65536u ? 65536u : wg))), dim3(256), 0, st, in, out, m, p.size);
    return hipGetLastError();
  }
  if (p.chunks > 1u)
  {
    hipLaunchKernelGGL((k_bitmmtf_reduce<E>), dim3(p.chunks), dim3(64), 0, st, in, m, p.chunkBytes, vals);
    hipLaunchKernelGGL((k_bitmmtf_scan<0>), dim3(1), dim3(1024), 0, st, vals, p.chunks);
  }
  hipLaunchKernelGGL((k_bitmmtf_apply<E>), dim3(p.chunks), dim3(64), 0, st, in, out, m, p.size, p.chunkBytes, p.chunks > 1u ? (const uint32_t *)vals : nullptr);
  return hipGetLastError();
}

hipError_t mmtf128_decode_segments_enqueue(const MmtfPlan &p, const uint8_t *dIn, uint8_t *ws, bool scan, hipStream_t st)
{
  if (p.S <= 1u) return hipSuccess;
  MmtfArgs a;
  a.in = dIn; a.out = nullptr;
  a.table = (uint32_t *)(ws + p.offTable);
  a.counts = (uint32_t *)(ws + p.offCounts);
  a.size = p.size; a.rows = p.rows; a.R = p.R; a.S = p.S;
  hipLaunchKernelGGL((k_mmtf_rows<16, true, false>), dim3((uint32_t)(((uint64_t)(a.S - 1u) * 16u + 63u) / 64u)), dim3(64), 0, st, a);
  if (scan) hipLaunchKernelGGL((k_mmtf_scan_dec<16>), dim3(16), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t mmtf_enqueue(const MmtfPlan &p, bool decode, const uint8_t *dIn, uint8_t *dOut, uint8_t *ws, hipStream_t st)
{
  if (p.E != 0u)
    return p.E == 1u ? bitmmtf_enqueue<1>(p, decode, dIn, dOut, (uint32_t *)(ws + p.offVals), st) : bitmmtf_enqueue<2>(p, decode, dIn, dOut, (uint32_t *)(ws + p.offVals), st);
  if (p.rows == 0u)
  {
    hipLaunchKernelGGL((k_mmtf_copy_small<0>), dim3(1), dim3(64), 0, st, dIn, dOut, p.size);
    return hipGetLastError();
  }
  MmtfArgs a;
  a.in = dIn; a.out = dOut;
  a.table = (uint32_t *)(ws + p.offTable);
  a.counts = (uint32_t *)(ws + p.offCounts);
  a.size = p.size; a.rows = p.rows; a.R = p.R; a.S = p.S;
  if (p.W == 16u) return decode ? mmtf_rows_enqueue<16, true>(a, st) : mmtf_rows_enqueue<16, false>(a, st);
  return decode ? mmtf_rows_enqueue<32, true>(a, st) : mmtf_rows_enqueue<32, false>(a, st);
}

}   // namespace hsrle
