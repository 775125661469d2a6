// hsrle_capi_sh.h -- part of hsrle_capi.hip: C ABI of the rle8_sh codec (include/hsrle.h section 5; reference: src/rle_sh.c, src/rle.h:455-458).
// The plans (tables, tuning) are made here on the host from the uncompressed size alone; inst_rle8sh.hip launches them (kernels:
// hsrle_rle8sh.hip.h).  No kernel here.  The host-pointer functions stage like every other family: one Staging.
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
  p.offState = p.offRec + ((16ull * ((uint64_t)p.maxRec + 1u) + 255u) & ~255ull);
  p.total = 256u + p.offState + ((8ull * ((uint64_t)p.maxRec + 1u) + 255u) & ~255ull);
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
  p.offEr = p.offItems + ((16ull * p.maxItems + 255u) & ~255ull);
  p.offBits = p.offEr + ((32ull * p.maxEr + 255u) & ~255ull);
  p.total = 256u + p.offBits + ((4ull * p.bitWords + 255u) & ~255ull);
  return true;
}

// A capacity that always suffices (include/hsrle.h has the derivation)
static uint64_t rle8sh_capacity(uint64_t inSize) { return inSize + inSize / 221u + 21u; }

static uint32_t rle8sh_compress_dropin(const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize)
{
  if (pIn == nullptr || pOut == nullptr || inSize == 0u || inSize > kShMaxIn || outSize < inSize + 8u)   // (the reference's own test: rle8_mmtf128_compress_bounds)
    return 0;
  const uint64_t need = hsrle_rle8_sh_workspace_size(0, inSize), cap = rle8sh_capacity(inSize);
  if (need == 0u || !device_ok())
    return 0;
  Staging s;
  if (!s.reserve(inSize, cap) || !s.reserve_ws(need) || !s.up(pIn, inSize))
    return 0;
  if (hsrle_rle8_sh_compress_dev_async(s.in, inSize, s.out, cap, s.status, s.status + 1, s.ws, s.wsSize, nullptr) != HSRLE_OK)
    return 0;
  uint32_t h[2] = { 0u, 1u };   // size, status
  if (!s.words(h, s.status, 2) || h[1] != HSRLE_RLE8_SH_DONE || h[0] == 0u || h[0] > outSize || !s.down(pOut, s.out, h[0]))
    return 0;
  return h[0];
}

static uint32_t rle8sh_decompress_dropin(const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize)
{
  if (pIn == nullptr || pOut == nullptr || inSize < 8u || outSize == 0u)
    return 0;
  uint32_t hdr[2];
  memcpy(hdr, pIn, 8);
  const uint32_t expectedOut = hdr[0], expectedIn = hdr[1];
  if (expectedOut > outSize || expectedIn > inSize || expectedOut == 0u || expectedOut > kShMaxIn || expectedIn < 13u)
    return 0;
  const uint64_t need = hsrle_rle8_sh_workspace_size(1, expectedOut);
  if (need == 0u || !device_ok())
    return 0;
  Staging s;
  if (!s.reserve(expectedIn, expectedOut) || !s.reserve_ws(need) || !s.up(pIn, expectedIn))
    return 0;
  if (hsrle_rle8_sh_decompress_dev_async(s.in, expectedIn, s.out, expectedOut, s.status, s.ws, s.wsSize, nullptr) != HSRLE_OK)
    return 0;
  uint32_t status = 1u;
  if (!s.words(&status, s.status, 1) || status != HSRLE_RLE8_SH_DONE || !s.down(pOut, s.out, expectedOut))
    return 0;
  return expectedOut;
}

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
  ShEncPlan p;
  if (dIn == nullptr || dOut == nullptr || dOutSize == nullptr || dStatus == nullptr || dWorkspace == nullptr || !rle8sh_enc_plan(inSize, p))
    return HSRLE_ERR_ARGUMENT;
  const uintptr_t a = (uintptr_t)dIn, b = (uintptr_t)dOut;
  if ((a < b + outCapacity && b < a + inSize) || (((uintptr_t)dOutSize | (uintptr_t)dStatus) & 3u) != 0u)
    return HSRLE_ERR_ARGUMENT;
  if (outCapacity < inSize + 8u || workspaceSize < p.total)
    return HSRLE_ERR_CAPACITY;
  uint8_t *ws = (uint8_t *)(((uintptr_t)dWorkspace + 255u) & ~(uintptr_t)255u);
  const uint32_t cap = outCapacity > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)outCapacity;
  return rle8sh_compress_enqueue(p, (const uint8_t *)dIn, (uint8_t *)dOut, cap, dOutSize, dStatus, ws, (hipStream_t)stream) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

int hsrle_rle8_sh_decompress_dev_async(const void *dStream, uint64_t streamSize, void *dOut, uint64_t outSize, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize,
                                       void *stream)
{
  ShPlan p;
  if (dStream == nullptr || dOut == nullptr || dStatus == nullptr || dWorkspace == nullptr || streamSize == 0u || !rle8sh_plan(outSize, p))
    return HSRLE_ERR_ARGUMENT;
  const uintptr_t a = (uintptr_t)dStream, b = (uintptr_t)dOut;
  if ((a < b + outSize && b < a + streamSize) || ((uintptr_t)dStatus & 3u) != 0u)
    return HSRLE_ERR_ARGUMENT;
  if (workspaceSize < p.total)
    return HSRLE_ERR_CAPACITY;
  uint8_t *ws = (uint8_t *)(((uintptr_t)dWorkspace + 255u) & ~(uintptr_t)255u);
  const uint32_t cap = streamSize > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)streamSize;
  return rle8sh_decompress_enqueue(p, (const uint8_t *)dStream, cap, (uint8_t *)dOut, dStatus, ws, (hipStream_t)stream) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

uint32_t rle8_sh_bounds(const uint32_t size) { return size > kShMaxIn ? 0u : size + 13u; }   // rle_sh.c:93-96
uint32_t rle8_sh_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return rle8sh_compress_dropin(pIn, inSize, pOut, outSize); }
uint32_t rle8_sh_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return rle8sh_decompress_dropin(pIn, inSize, pOut, outSize); }

}   // extern "C"
