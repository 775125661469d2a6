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

// The entry index of one rle8_mmtf128 stream (kernels: hsrle_rle8mmtf_index.hip.h; launched by inst_rle8mmtfi.hip).  index_emit: behind compress_enqueue of the
// same plan, workspace and stream.  index_build: one wave, no workspace.  decompress_indexed: the decode plan and workspace of decompress_enqueue; streamSize,
// spacing, entries: the index header the caller holds.
hipError_t rle8mmtf_index_emit_enqueue(const Rle8MmtfPlan &p, uint8_t *dOut, uint32_t *dOutSize, uint8_t *ws, uint32_t spacing, uint8_t *dIndex, uint64_t *dIndexSize, hipStream_t st);
hipError_t rle8mmtf_index_build_enqueue(const uint8_t *dStream, uint32_t streamCap, uint32_t size, uint32_t spacing, uint8_t *dIndex, uint64_t *dIndexSize, uint32_t *dStatus,
                                        hipStream_t st);
hipError_t rle8mmtf_decompress_indexed_enqueue(const Rle8MmtfPlan &p, const uint8_t *dStream, uint32_t streamCap, const uint8_t *dIndex, uint32_t streamSize, uint32_t spacing,
                                               uint32_t entries, uint8_t *dOut, uint32_t *dStatus, uint8_t *ws, hipStream_t st);

// The first two launches of decompress_indexed and its third: the whole stream's rank buffer and ctrl[0] (the verdict, also in *dStatus), ctrl[3] (the stream's size).
hipError_t rle8mmtf_expand_indexed_enqueue(const Rle8MmtfPlan &p, const uint8_t *dStream, uint32_t streamCap, const uint8_t *dIndex, uint32_t streamSize, uint32_t spacing,
                                           uint32_t entries, uint32_t *dStatus, uint8_t *ws, hipStream_t st);
// mmtf128 decode without its last pass (inst_mmtf.hip): pass A, and with `scan` pass B, which leaves the list in front of segment s in slot s of the state table.
// Nothing for a plan of one segment.
hipError_t mmtf128_decode_segments_enqueue(const MmtfPlan &p, const uint8_t *dIn, uint8_t *ws, bool scan, hipStream_t st);

// Checkpoints and byte-range decode of one rle8_mmtf128 stream (kernels: hsrle_rle8mmtf_range.hip.h; launched by inst_rle8mmtfr.hip).  checkpoints_build: the decode
// plan and workspace of decompress_enqueue.  decompress_range: rows [c, r1) are decoded from the checkpoint of row c (c = 0: from the identity) and output bytes
// [skip, skip + length) of them copied out.  Workspace, from its 256-byte aligned start: control words, the rank buffer of the rows, the packet records, the staging
// area, the workspace of the mmtf128 plan of the rows.
struct RmRangePlan
{
  MmtfPlan mmtf;                    // of the r1 - c rows, and the tail bytes if r1 = R
  uint32_t size = 0, R = 0;         // the whole stream: uncompressed bytes, rows
  uint32_t c = 0, r1 = 0;
  uint32_t maxRec = 0;              // records the table holds
  uint32_t stretches = 0;           // a bound on the stretches that reach into [c, r1): the walk's grid
  uint64_t skip = 0;
  uint64_t offRanks = 0, offRec = 0, offStage = 0, offMmtf = 0, total = 0;
};
hipError_t rle8mmtf_checkpoints_build_enqueue(const Rle8MmtfPlan &p, const uint8_t *dStream, uint32_t streamCap, const uint8_t *dIndex, uint32_t streamSize, uint32_t spacing,
                                              uint32_t entries, uint32_t checkpointRows, uint32_t count, uint8_t *dCheckpoints, uint64_t *dSize, uint32_t *dStatus, uint8_t *ws,
                                              hipStream_t st);
hipError_t rle8mmtf_decompress_range_enqueue(const RmRangePlan &p, const uint8_t *dStream, uint32_t streamCap, const uint8_t *dIndex, uint32_t streamSize, uint32_t spacing,
                                             uint32_t entries, const uint8_t *dCheckpoints, uint32_t checkpointRows, uint32_t count, uint8_t *dOut, uint64_t length,
                                             uint32_t *dStatus, uint8_t *ws, hipStream_t st);

// The blocked form (hsrle_capi_mmtfb.h plans, inst_rle8mmtfb.hip launches, kernels: hsrle_rle8mmtfb.hip.h).  Workspace, from its 256-byte aligned start:
// 256 bytes of words for the whole call, then `inFlight` SLOTS: control words, the block's rank buffer, then -- encode: the span summaries and the span
// results of a block; decode: its packet records.
struct MfbPlan
{
  uint64_t size = 0;                // uncompressed bytes of the whole container
  uint32_t blockSize = 0, blockCount = 0;
  uint32_t inFlight = 0;            // blocks per group: min(blocks of the call, blocks in flight)
  uint32_t SP = 0, maxRec = 0;      // encode: rows per span; decode: records a slot can hold
  uint64_t offRanks = 0, offA = 0, offB = 0;   // inside a slot; A: summaries / records, B: results
  uint64_t encSlot = 0, decSlot = 0;
};
hipError_t rle8mmtfb_compress_enqueue(const MfbPlan &p, const uint8_t *dIn, uint8_t *dOut, uint64_t outCap, uint64_t *dOutSize, uint32_t *dStatus, uint8_t *ws, hipStream_t st);
hipError_t rle8mmtfb_decompress_enqueue(const MfbPlan &p, const uint8_t *dContainer, uint64_t payloadSize, uint32_t firstBlock, uint32_t blockCount, uint8_t *dOut,
                                        uint32_t *dStatus, uint8_t *ws, hipStream_t st);

}   // namespace hsrle
