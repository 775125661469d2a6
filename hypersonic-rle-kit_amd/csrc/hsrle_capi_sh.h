// hsrle_capi_sh.h -- part of hsrle_capi.hip: C ABI of the rle8_sh codec (include/hsrle.h section 5; reference: src/rle_sh.c, src/rle.h:455-458).
// The plans (tables, tuning) are made here on the host from the uncompressed size alone; inst_rle8sh.hip launches them (kernels:
// hsrle_rle8sh.hip.h).  No kernel here.  Device entries and host-pointer functions are the single-stream codecs' shared ones (hsrle_capi_host.h).
#pragma once
#include "hsrle_capi_host.h"
#include "hsrle_rle8sh.h"

namespace hsrle {

static std::atomic<uint32_t> g_shStretchSymbols{ 0 }, g_shWalkWindow{ 0 }, g_shSerialState{ 0 };
constexpr uint32_t kShMaxIn = 1u << 30;
constexpr uint32_t kShStretchSymbols = 128u, kShStretchMax = 4096u;
constexpr uint32_t kShWindow = 1024u, kShWindowMin = 64u;   // == kShWinMax / kShWinMin of the kernels

static bool rle8sh_plan(uint64_t size, ShPlan &p)
{
  if (size == 0u || size > kShMaxIn)
    return false;
  const uint32_t cap = g_shStretchSymbols.load(), win = g_shWalkWindow.load() & ~15u;
  p.size = (uint32_t)size;
  p.maxRec = p.size;
  p.cap = cap == 0u || cap > kShStretchMax ? kShStretchSymbols : cap;
  p.win = win < kShWindowMin || win > kShWindow ? kShWindow : win;
  p.force = g_shSerialState.load() != 0u ? 1u : 0u;
  p.offRec = 256u;
  p.offState = p.offRec + align_up(16ull * ((uint64_t)p.maxRec + 1u), 256);
  p.total = 256u + p.offState + align_up(8ull * ((uint64_t)p.maxRec + 1u), 256);
  return true;
}

// Encode tables.  An item needs a run of 10 and more bytes (a change of R) or of 15 and more bytes of R (a FILL) and such a run gives at most two items
// (the block in front of it and its own), so 2 * size / 11 items at the most; an encoded copy adds an emission record per 416 bytes and one for its
// rest.  Bits: 4 per byte at the most (T) and 7 per record.
static bool rle8sh_enc_plan(uint64_t size, ShEncPlan &p)
{
  if (size == 0u || size > kShMaxIn)
    return false;
  p.size = (uint32_t)size;
  p.maxItems = p.size / 5u + 8u;
  p.maxEr = p.maxItems + p.size / 256u + 8u;
  p.bitWords = (p.size / 2u + p.maxEr + 16u) / 4u + 1u;
  p.offItems = 256u;
  p.offEr = p.offItems + align_up(16ull * p.maxItems, 256);
  p.offBits = p.offEr + align_up(32ull * p.maxEr, 256);
  p.total = 256u + p.offBits + align_up(4ull * p.bitWords, 256);
  return true;
}

// A capacity that always suffices (include/hsrle.h has the derivation)
static uint64_t rle8sh_capacity(uint64_t inSize) { return inSize + inSize / 221u + 21u; }

static const StreamCodec kRle8ShCodec = { hsrle_rle8_sh_workspace_size, hsrle_rle8_sh_compress_dev_async, hsrle_rle8_sh_decompress_dev_async, kShMaxIn, 13u, HSRLE_RLE8_SH_DONE };

}   // namespace hsrle

extern "C" {

void hsrle_rle8_sh_tuning(uint32_t stretchSymbols, uint32_t walkWindow, uint32_t serialState)
{
  g_shStretchSymbols.store(stretchSymbols);
  g_shWalkWindow.store(walkWindow);
  g_shSerialState.store(serialState);
}

uint64_t hsrle_rle8_sh_workspace_size(int decode, uint64_t size)
{
  ShPlan p;
  ShEncPlan e;
  if (decode != 0)
    return rle8sh_plan(size, p) ? p.total : 0u;
  return rle8sh_enc_plan(size, e) ? e.total : 0u;
}

uint64_t hsrle_rle8_sh_capacity(uint64_t inSize) { return inSize == 0u || inSize > kShMaxIn ? 0u : rle8sh_capacity(inSize); }

int hsrle_rle8_sh_compress_dev_async(const void *dIn, uint64_t inSize, void *dOut, uint64_t outCapacity, uint32_t *dOutSize, uint32_t *dStatus, void *dWorkspace,
                                     uint64_t workspaceSize, void *stream)
{
  return stream_compress_entry<ShEncPlan>(rle8sh_enc_plan, rle8sh_compress_enqueue, dIn, inSize, dOut, outCapacity, dOutSize, dStatus, dWorkspace, workspaceSize, stream);
}

int hsrle_rle8_sh_decompress_dev_async(const void *dStream, uint64_t streamSize, void *dOut, uint64_t outSize, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize,
                                       void *stream)
{
  return stream_decompress_entry<ShPlan>(rle8sh_plan, rle8sh_decompress_enqueue, dStream, streamSize, dOut, outSize, dStatus, dWorkspace, workspaceSize, stream);
}

uint32_t rle8_sh_bounds(const uint32_t size) { return size > kShMaxIn ? 0u : size + 13u; }   // rle_sh.c:93-96
uint32_t rle8_sh_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize)
{
  return stream_compress_dropin(kRle8ShCodec, rle8sh_capacity(inSize), rle8sh_capacity(inSize), pIn, inSize, pOut, outSize);
}
uint32_t rle8_sh_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return stream_decompress_dropin(kRle8ShCodec, pIn, inSize, pOut, outSize); }

}   // extern "C"
