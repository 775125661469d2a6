// hsrle_rle8sh.h -- host side of the rle8_sh codec: what hsrle_capi_sh.h (a part of hsrle_capi.hip) plans and inst_rle8sh.hip launches
// (kernels: hsrle_rle8sh.hip.h).  Workspace, from its 256-byte aligned start: control words, then -- decode: the record table, summary and state (8 bytes) of
// every record; encode: the item table, the emission records, the bit buffer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hsrle {

struct ShPlan
{
  uint32_t size = 0;
  uint32_t maxRec = 0;              // every record holds at least one output byte: `size` records at the most
  uint32_t cap = 0, win = 0;        // symbols per stretch record, bytes per walk window
  uint32_t force = 0;               // 1: the serial symbol pass instead of the scan under the guess
  uint64_t offRec = 0, offState = 0, total = 0;
};

struct ShEncPlan
{
  uint32_t size = 0;
  uint32_t maxItems = 0, maxEr = 0, bitWords = 0;
  uint64_t offItems = 0, offEr = 0, offBits = 0, total = 0;
};

// enqueue-only: kernels on `st`, nothing else
hipError_t rle8sh_compress_enqueue(const ShEncPlan &p, const uint8_t *dIn, uint8_t *dOut, uint32_t outCap, uint32_t *dOutSize, uint32_t *dStatus, uint8_t *ws, hipStream_t st);
hipError_t rle8sh_decompress_enqueue(const ShPlan &p, const uint8_t *dStream, uint32_t streamCap, uint8_t *dOut, uint32_t *dStatus, uint8_t *ws, hipStream_t st);

// The blocked form (hsrle_capi_shb.h plans, inst_rle8shb.hip launches, kernels: hsrle_rle8shb.hip.h).  Workspace, from its 256-byte aligned start: 256 bytes
// of words for the whole call, then `inFlight` SLOTS, each the workspace of a single stream of blockSize bytes (enc.total / dec.total).
struct ShbPlan
{
  uint64_t size = 0;                // uncompressed bytes of the whole container
  uint32_t blockSize = 0, blockCount = 0;
  uint32_t inFlight = 0;            // blocks per group: min(blocks of the call, blocks in flight)
  ShEncPlan enc;                    // of ONE block
  ShPlan dec;
  uint64_t total = 0;
};

hipError_t rle8shb_compress_enqueue(const ShbPlan &p, const uint8_t *dIn, uint8_t *dOut, uint64_t outCap, uint64_t *dOutSize, uint32_t *dStatus, uint8_t *ws, hipStream_t st);
hipError_t rle8shb_decompress_enqueue(const ShbPlan &p, const uint8_t *dContainer, uint64_t payloadSize, uint32_t firstBlock, uint32_t blockCount, uint8_t *dOut,
                                      uint32_t *dStatus, uint8_t *ws, hipStream_t st);

}   // namespace hsrle
