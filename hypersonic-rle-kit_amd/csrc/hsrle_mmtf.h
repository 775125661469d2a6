// hsrle_mmtf.h -- host side of the mmtf / bitmmtf transforms: what hsrle_mmtf_capi.hip plans and inst_mmtf.hip launches (kernels: hsrle_mmtf.hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hsrle {

struct MmtfPlan
{
  uint32_t W = 0, E = 0;            // mmtf: W = 16 / 32 (E = 0); bitmmtf: E = 1 / 2 (W = 0)
  uint32_t size = 0;
  uint32_t rows = 0, R = 0, S = 0;  // mmtf: size / W rows in S segments of R
  uint32_t chunkBytes = 0, chunks = 0;   // bitmmtf decode
  uint64_t offCounts = 0, offTable = 0, offVals = 0, total = 0;   // workspace (offsets from its 256-byte aligned start; total includes that slack)
};

// enqueue-only: kernels on `st`, nothing else
hipError_t mmtf_enqueue(const MmtfPlan &p, bool decode, const uint8_t *dIn, uint8_t *dOut, uint8_t *ws, hipStream_t st);

}   // namespace hsrle
