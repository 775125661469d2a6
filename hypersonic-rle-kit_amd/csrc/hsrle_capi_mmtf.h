// hsrle_capi_mmtf.h -- part of hsrle_capi.hip: C ABI of the mmtf / bitmmtf transforms (include/hsrle.h section 5; reference: src/rle.h:420-438, src/mmtf.c, src/bit_mmtf.c).
// The plan (segment length, chunk length, workspace layout) is made here on the host from the size alone; inst_mmtf.hip launches it.
// Behind it: the C ABI of the rle8_mmtf128 codec (reference: src/rle8_mmtf.c, src/rle.h:442-452), which runs the mmtf128 plan between its own passes
// (kernels: hsrle_rle8mmtf.hip.h, launched by inst_rle8mmtf.hip).  No kernel here.  The host-pointer functions take the staged trip of hsrle_capi_host.h;
// rle8_mmtf128's device entries and host-pointer functions are the single-stream codecs' shared ones (hsrle_capi_host.h).
#pragma once
#include "hsrle_capi_host.h"
#include "hsrle_mmtf.h"

#include <math.h>

namespace hsrle {

static std::atomic<uint32_t> g_mmtfSegmentRows{ 0 };

static uint32_t isqrt32(uint32_t v)
{
  uint32_t r = (uint32_t)sqrt((double)v);
  while ((uint64_t)r * r > v) r--;
  while ((uint64_t)(r + 1u) * (r + 1u) <= v) r++;
  return r;
}
static inline uint64_t min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

constexpr uint32_t kMmtfLanes = 131072u;    // (segment, column) lanes that fill the device: 256 CUs x 8 resident waves x 64
constexpr uint32_t kMmtfMinRows = 256u;     // a segment's state is 256 bytes per column: never more state than input
constexpr uint32_t kBitChunks = 8192u, kBitMinChunk = 4096u;
constexpr uint32_t kBitMaxChunks = 1u << 24;

// With the library's own choice (tuning 0) the workspace is sized from BOUNDS of the segment / chunk count that grow with the size
// (the counts themselves do not: the segment length is rounded), so hsrle_mmtf_workspace_size is monotone.
static bool mmtf_plan(int transform, uint64_t size, MmtfPlan &p)
{
  if (transform < HSRLE_MMTF128 || transform > HSRLE_BITMMTF16 || size > 0xFFFFFFFFull)
    return false;
  const uint32_t tuning = g_mmtfSegmentRows.load();
  p.size = (uint32_t)size;
  if (transform <= HSRLE_MMTF256)
  {
    const uint32_t W = transform == HSRLE_MMTF128 ? 16u : 32u, target = kMmtfLanes / W;
    p.W = W;
    p.rows = p.size / W;
    uint64_t segBound;
    if (tuning != 0u)
    {
      p.R = tuning;
      p.S = (uint32_t)(((uint64_t)p.rows + p.R - 1u) / p.R);
      segBound = p.S;
    }
    else
    {
      const uint32_t root = isqrt32(p.rows);
      uint32_t R = (p.rows + target - 1u) / target;
      if (R < root) R = root;
      if (R < kMmtfMinRows) R = kMmtfMinRows;
      p.R = (R + 15u) & ~15u;   // whole 16-row tiles
      p.S = (p.rows + p.R - 1u) / p.R;
      segBound = min64(min64(target, (uint64_t)p.rows / kMmtfMinRows + 1u), (uint64_t)root + 3u);
    }
    const uint64_t groups = (segBound * W + 63u) / 64u;
    p.offCounts = 0;
    p.offTable = groups * 256u;
    p.total = 256u + p.offTable + groups * 16384u;
    return true;
  }
  const uint32_t E = transform == HSRLE_BITMMTF8 ? 1u : 2u, m = p.size & ~(E - 1u);
  p.E = E;
  uint64_t chunkBound;
  uint64_t cb;
  if (tuning != 0u)
  {
    cb = (uint64_t)tuning * E;
    while (((uint64_t)m + cb - 1u) / cb > kBitMaxChunks) cb *= 2u;   // (a launch has a grid limit; the knob is for tests)
    if (cb > 0x80000000ull) cb = 0x80000000ull;
    chunkBound = ((uint64_t)m + cb - 1u) / cb;
  }
  else
  {
    cb = (((uint64_t)m + kBitChunks - 1u) / kBitChunks + 1023u) & ~1023ull;
    if (cb < kBitMinChunk) cb = kBitMinChunk;
    chunkBound = min64(kBitChunks, (uint64_t)m / kBitMinChunk + 1u);
  }
  p.chunkBytes = (uint32_t)cb;
  p.chunks = (uint32_t)(((uint64_t)m + cb - 1u) / cb);
  if (p.chunks == 0u) p.chunks = 1u;
  if (chunkBound == 0u) chunkBound = 1u;
  p.offVals = 0;
  p.total = 256u + align_up(4u * chunkBound, 256);
  return true;
}

// ---- the host-pointer functions: the staged trip (hsrle_capi_host.h), so they run one after the other with every other drop-in call on the device ----
static uint32_t mmtf_dropin(int transform, int decode, const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize)
{
  if (pIn == nullptr || pOut == nullptr || inSize == 0u || inSize > outSize)   // (mmtf.c does not look at the pointers; a NULL here is a 0, not a fault)
    return 0;
  const uint64_t need = hsrle_mmtf_workspace_size(transform, inSize);
  if (need == 0u || !device_ok())
    return 0;
  uint64_t size = 0;
  const int rc = staged_call(
    pIn, inSize, inSize, need, pOut, 0u, [&](Staging &s) { return hsrle_mmtf_dev_async(transform, decode, s.in, inSize, s.out, s.ws, s.wsSize, nullptr); },
    [&](const uint32_t *, uint64_t &n) { n = inSize; return (int)HSRLE_OK; }, &size);
  return rc == HSRLE_OK ? inSize : 0u;
}

// ---- rle8_mmtf128 (reference: src/rle8_mmtf.c): the mmtf128 plan above between the codec's own passes ----
static std::atomic<uint32_t> g_rle8MmtfSpanRows{ 0 };
constexpr uint32_t kRle8MmtfMaxIn = 1u << 30;

static bool rle8mmtf_plan(int decode, uint64_t size, Rle8MmtfPlan &p)
{
  if (size == 0u || size > kRle8MmtfMaxIn || !mmtf_plan(HSRLE_MMTF128, size, p.mmtf))
    return false;
  p.size = (uint32_t)size;
  p.rows = p.size / 16u;
  const uint32_t tuning = g_rle8MmtfSpanRows.load();
  p.SP = tuning == 0u || tuning > 64u ? 64u : tuning;
  p.spans = (p.rows + p.SP - 1u) / p.SP;
  p.maxRec = p.rows + 1u;   // a record per non-null packet, and such a packet holds a row
  p.offRanks = 256u;
  p.offA = p.offRanks + align_up((uint64_t)p.size + 16u, 256);
  p.offB = p.offA + align_up(16ull * (decode ? p.maxRec : p.spans), 256);
  p.offMmtf = p.offB + align_up(decode ? 0u : 16ull * p.spans, 256);
  p.total = 256u + p.offMmtf + p.mmtf.total;
  return true;
}

static uint32_t rle8mmtf_bounds(uint32_t inSize) { return inSize > kRle8MmtfMaxIn ? 0u : inSize + 8u; }   // rle8_mmtf.c:26-32

static bool rle8mmtf_enc_plan(uint64_t size, Rle8MmtfPlan &p) { return rle8mmtf_plan(0, size, p); }
static bool rle8mmtf_dec_plan(uint64_t size, Rle8MmtfPlan &p) { return rle8mmtf_plan(1, size, p); }

static const StreamCodec kRle8MmtfCodec = { hsrle_rle8_mmtf128_workspace_size, hsrle_rle8_mmtf128_compress_dev_async, hsrle_rle8_mmtf128_decompress_dev_async, kRle8MmtfMaxIn, 8u,
                                            HSRLE_RLE8_MMTF_DONE };

}   // namespace hsrle

extern "C" {

void hsrle_rle8_mmtf_tuning(uint32_t spanRows) { g_rle8MmtfSpanRows.store(spanRows); }

uint64_t hsrle_rle8_mmtf128_workspace_size(int decode, uint64_t size)
{
  Rle8MmtfPlan p;
  return rle8mmtf_plan(decode != 0, size, p) ? p.total : 0u;
}

int hsrle_rle8_mmtf128_compress_dev_async(const void *dIn, uint64_t inSize, void *dOut, uint64_t outCapacity, uint32_t *dOutSize, uint32_t *dStatus, void *dWorkspace,
                                          uint64_t workspaceSize, void *stream)
{
  return stream_compress_entry<Rle8MmtfPlan>(rle8mmtf_enc_plan, rle8mmtf_compress_enqueue, dIn, inSize, dOut, outCapacity, dOutSize, dStatus, dWorkspace, workspaceSize, stream);
}

int hsrle_rle8_mmtf128_decompress_dev_async(const void *dStream, uint64_t streamSize, void *dOut, uint64_t outSize, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize,
                                            void *stream)
{
  return stream_decompress_entry<Rle8MmtfPlan>(rle8mmtf_dec_plan, rle8mmtf_decompress_enqueue, dStream, streamSize, dOut, outSize, dStatus, dWorkspace, workspaceSize, stream);
}

uint32_t rle8_mmtf128_compress_bounds(const uint32_t inSize) { return rle8mmtf_bounds(inSize); }
uint32_t rle8_mmtf256_compress_bounds(const uint32_t inSize) { return rle8mmtf_bounds(inSize); }
uint32_t rle8_mmtf128_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize)
{
  return stream_compress_dropin(kRle8MmtfCodec, inSize, (uint64_t)inSize + 64u, pIn, inSize, pOut, outSize);
}
uint32_t rle8_mmtf128_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return stream_decompress_dropin(kRle8MmtfCodec, pIn, inSize, pOut, outSize); }

void hsrle_mmtf_tuning(uint32_t segmentRows) { g_mmtfSegmentRows.store(segmentRows); }

uint64_t hsrle_mmtf_workspace_size(int transform, uint64_t size)
{
  MmtfPlan p;
  return mmtf_plan(transform, size, p) ? p.total : 0u;
}

int hsrle_mmtf_dev_async(int transform, int decode, const void *dIn, uint64_t size, void *dOut, void *dWorkspace, uint64_t workspaceSize, void *stream)
{
  MmtfPlan p;
  if (!mmtf_plan(transform, size, p))
    return HSRLE_ERR_ARGUMENT;
  if (size == 0u)
    return HSRLE_OK;
  if (dIn == nullptr || dOut == nullptr || dWorkspace == nullptr)
    return HSRLE_ERR_ARGUMENT;
  if (ranges_overlap(dIn, size, dOut, size))
    return HSRLE_ERR_ARGUMENT;
  if (workspaceSize < p.total)
    return HSRLE_ERR_CAPACITY;
  return mmtf_enqueue(p, decode != 0, (const uint8_t *)dIn, (uint8_t *)dOut, workspace_start(dWorkspace), (hipStream_t)stream) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

uint32_t mmtf_bounds(const uint32_t inSize) { return inSize; }       // mmtf.c
uint32_t bitmmtf_bounds(const uint32_t inSize) { return inSize; }    // bit_mmtf.c

#define HSRLE_MMTF_DROPIN(name, id) \
  uint32_t name##_encode(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mmtf_dropin(id, 0, pIn, inSize, pOut, outSize); } \
  uint32_t name##_decode(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mmtf_dropin(id, 1, pIn, inSize, pOut, outSize); }
HSRLE_MMTF_DROPIN(mmtf128, HSRLE_MMTF128)
HSRLE_MMTF_DROPIN(mmtf256, HSRLE_MMTF256)
HSRLE_MMTF_DROPIN(bitmmtf8, HSRLE_BITMMTF8)
HSRLE_MMTF_DROPIN(bitmmtf16, HSRLE_BITMMTF16)
#undef HSRLE_MMTF_DROPIN

}   // extern "C"
