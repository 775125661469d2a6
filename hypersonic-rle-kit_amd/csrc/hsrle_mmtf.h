// hsrle_mmtf.h -- host side of the mmtf / bitmmtf transforms: what hsrle_capi_mmtf.h (a part of hsrle_capi.hip) plans and inst_mmtf.hip launches (kernels: hsrle_mmtf.hip.h).
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

// rle8_mmtf128 (kernels: hsrle_rle8mmtf.hip.h; launched by inst_rle8mmtf.hip).  Workspace, from its 256-byte aligned start: control words, the rank
// buffer, table A (encode: the span summaries; decode: the packet records), table B (encode: the span results), the mmtf128 plan's workspace.
struct Rle8MmtfPlan
{
  MmtfPlan mmtf;
  uint32_t size = 0, rows = 0;
  uint32_t SP = 0, spans = 0;       // encode: rows per span (<= 64), spans
  uint32_t maxRec = 0;              // decode: records table A can hold
  uint64_t offRanks = 0, offA = 0, offB = 0, offMmtf = 0, total = 0;
};
hipError_t rle8mmtf_compress_enqueue(const Rle8MmtfPlan &p, const uint8_t *dIn, uint8_t *dOut, uint32_t outCap, uint32_t *dOutSize, uint32_t *dStatus, uint8_t *ws, hipStream_t st);
hipError_t rle8mmtf_decompress_enqueue(const Rle8MmtfPlan &p, const uint8_t *dStream, uint32_t streamCap, uint8_t *dOut, uint32_t *dStatus, uint8_t *ws, hipStream_t st);

}   // namespace hsrle
