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

// ---- the entry index of an rle8_mmtf128 stream (kernels and layout: hsrle_rle8mmtf_index.hip.h) ----
constexpr uint32_t kRmIndexDefaultSpacing = 1024u;   // rows: the fastest of 256 / 1024 / 4096 on the video-shaped 1 GiB decode (profiles/r18_rle8_mmtf_index.md)
constexpr uint32_t kRmIndexCodec = HSRLE_RLE8_MMTF_INDEX_CODEC;   // hsrle_mono_index_info_t::codec of such an index: no id of the codec table

// spacingRows as the calls take it -> rows per window, 0 = not a spacing
static uint32_t rm_index_spacing(uint32_t spacingRows)
{
  if (spacingRows == 0u) return kRmIndexDefaultSpacing;
  return (spacingRows % 64u != 0u || spacingRows > (1u << 20)) ? 0u : spacingRows;
}
// windows 1 .. of `spacing` rows that hold a row: the most entries
static uint32_t rm_index_max_entries(uint64_t uncompressedSize, uint32_t spacing)
{
  const uint64_t rows = uncompressedSize / 16u;
  return rows == 0u ? 0u : (uint32_t)((rows - 1u) / spacing);
}
static uint64_t rm_index_bound(uint64_t uncompressedSize, uint32_t spacingRows)
{
  const uint32_t spacing = rm_index_spacing(spacingRows);
  return (spacing == 0u || uncompressedSize > kRle8MmtfMaxIn) ? 0u : 64u + 16ull * rm_index_max_entries(uncompressedSize, spacing);
}
// what a caller's header has to say before anything is planned from it (a size that does not go with the count: left to the device's comparison, INDEX)
static bool rm_index_info_ok(const hsrle_mono_index_info_t &i)
{
  return i.version == 1u && i.codec == kRmIndexCodec && i.recordBytes == 16u && i.spacing != 0u && rm_index_spacing(i.spacing) == i.spacing && i.uncompressedSize != 0u &&
         i.uncompressedSize <= kRle8MmtfMaxIn && i.recordCount <= rm_index_max_entries(i.uncompressedSize, i.spacing);
}
static bool rm_index_args_ok(const void *dIndex, uint64_t *dIndexSize) { return dIndex != nullptr && dIndexSize != nullptr && word_aligned(dIndexSize, 8); }

// ---- checkpoints and byte-range decode of an rle8_mmtf128 stream (kernels and layout: hsrle_rle8mmtf_range.hip.h) ----
constexpr uint32_t kRmCheckpointDefaultRows = 65536u;   // 1 MiB of output per checkpoint: the sidecar is 0.39 % of the uncompressed size

// checkpointRows as the calls take it -> rows per checkpoint, 0 = not a value
static uint32_t rm_checkpoint_rows(uint32_t checkpointRows)
{
  if (checkpointRows == 0u) return kRmCheckpointDefaultRows;
  return (checkpointRows % 64u != 0u || checkpointRows > (1u << 24)) ? 0u : checkpointRows;
}
static uint32_t rm_checkpoint_count(uint64_t uncompressedSize, uint32_t rows)
{
  const uint64_t R = uncompressedSize / 16u;
  return R == 0u ? 0u : (uint32_t)((R - 1u) / rows);
}
static uint64_t rm_checkpoints_bound(uint64_t uncompressedSize, uint32_t checkpointRows)
{
  const uint32_t rows = rm_checkpoint_rows(checkpointRows);
  return (rows == 0u || uncompressedSize > kRle8MmtfMaxIn) ? 0u : 64u + 4096ull * rm_checkpoint_count(uncompressedSize, rows);
}
static bool rm_checkpoints_info_ok(const hsrle_rle8_mmtf128_checkpoints_info_t &i)
{
  return i.version == 1u && i.headerBytes == 64u && i.checkpointRows != 0u && rm_checkpoint_rows(i.checkpointRows) == i.checkpointRows && i.uncompressedSize != 0u &&
         i.uncompressedSize <= kRle8MmtfMaxIn && i.streamSize >= 10u && i.checkpointCount == rm_checkpoint_count(i.uncompressedSize, i.checkpointRows) &&
         i.size == 64u + 4096ull * i.checkpointCount;
}

// the workspace of `rows` rows (and `tail` bytes behind them) at an index spacing
static bool rm_range_layout(uint32_t rows, uint32_t tail, uint32_t spacing, RmRangePlan &p)
{
  if (!mmtf_plan(HSRLE_MMTF128, (uint64_t)rows * 16u + tail, p.mmtf))
    return false;
  p.maxRec = rows + 2u * spacing + 1u;   // packets of an index by the rule: at most `spacing` between e0 and row c, a row each inside, `spacing` behind r1 in the last stretch
  p.offRanks = 256u;
  p.offRec = p.offRanks + align_up((uint64_t)rows * 16u + 16u, 256);
  p.offStage = p.offRec + align_up(16ull * p.maxRec, 256);
  p.offMmtf = p.offStage + align_up((uint64_t)rows * 16u + 16u, 256);
  p.total = 256u + p.offMmtf + p.mmtf.total;
  return true;
}
// the most rows a range of `length` bytes decodes: up to checkpointRows - 1 in front of its first row
static uint32_t rm_range_max_rows(uint64_t length, uint32_t checkpointRows) { return checkpointRows + (uint32_t)((length + 30u) / 16u); }

// rows [c, r1) of a stream of `size` bytes for output bytes [offset, offset + length), length != 0, offset + length <= size
static bool rm_range_plan(uint64_t size, uint64_t offset, uint64_t length, uint32_t spacing, uint32_t checkpointRows, RmRangePlan &p)
{
  const uint32_t R = (uint32_t)(size / 16u);
  const uint64_t r0 = offset / 16u, first = R == 0u ? 0u : min64(r0, R - 1u);   // (a range of tail bytes alone: through the last row)
  p.size = (uint32_t)size;
  p.R = R;
  p.c = (uint32_t)(first / checkpointRows) * checkpointRows;
  p.r1 = (uint32_t)min64(R, (offset + length + 15u) / 16u);
  p.skip = offset - 16ull * p.c;
  p.stretches = (p.r1 - p.c) / spacing + 3u;   // e0's, and an entry per window that (c, r1) touches
  return rm_range_layout(p.r1 - p.c, p.r1 == R ? p.size - 16u * R : 0u, spacing, p);
}

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

uint64_t hsrle_rle8_mmtf128_index_bound(uint64_t uncompressedSize, uint32_t spacingRows) { return rm_index_bound(uncompressedSize, spacingRows); }

int hsrle_rle8_mmtf128_index_info_host(const void *pIndex, uint64_t size, hsrle_mono_index_info_t *pInfo)
{
  if (pIndex == nullptr || pInfo == nullptr)
    return HSRLE_ERR_ARGUMENT;
  uint32_t w[16];
  if (size < sizeof(w))
    return HSRLE_ERR_FORMAT;
  memcpy(w, pIndex, sizeof(w));
  hsrle_mono_index_info_t i = {};
  i.version = w[2]; i.codec = kRmIndexCodec;
  i.uncompressedSize = w[4]; i.compressedSize = w[5];
  i.spacing = w[6]; i.recordCount = w[7]; i.recordBytes = 16u;
  i.indexBytes = (uint64_t)w[8] | (uint64_t)w[9] << 32;
  bool zeros = true;
  for (int k = 10; k < 16; k++) zeros = zeros && w[k] == 0u;
  if (memcmp(w, "HSRLEMFI", 8) != 0 || w[3] != 64u || !zeros || !rm_index_info_ok(i) || i.indexBytes != 64u + 16ull * i.recordCount || i.compressedSize < 10u || i.indexBytes > size)
    return HSRLE_ERR_FORMAT;
  *pInfo = i;
  return HSRLE_OK;
}

int hsrle_rle8_mmtf128_compress_indexed_dev_async(const void *dIn, uint64_t inSize, void *dOut, uint64_t outCapacity, uint32_t *dOutSize, uint32_t *dStatus, void *dWorkspace,
                                                  uint64_t workspaceSize, uint32_t spacingRows, void *dIndex, uint64_t indexCapacity, uint64_t *dIndexSize, void *stream)
{
  Rle8MmtfPlan p;
  const int rc = stream_compress_check(rle8mmtf_enc_plan, dIn, inSize, dOut, outCapacity, dOutSize, dStatus, dWorkspace, workspaceSize, p);
  const uint32_t spacing = rm_index_spacing(spacingRows);
  if (rc == HSRLE_ERR_ARGUMENT || spacing == 0u || !rm_index_args_ok(dIndex, dIndexSize) || ranges_overlap(dIndex, indexCapacity, dIn, inSize) ||
      ranges_overlap(dIndex, indexCapacity, dOut, outCapacity))
    return HSRLE_ERR_ARGUMENT;
  if (rc != HSRLE_OK || indexCapacity < rm_index_bound(inSize, spacing))
    return HSRLE_ERR_CAPACITY;
  uint8_t *ws = workspace_start(dWorkspace);
  hipStream_t st = (hipStream_t)stream;
  if (rle8mmtf_compress_enqueue(p, (const uint8_t *)dIn, (uint8_t *)dOut, clamp32(outCapacity), dOutSize, dStatus, ws, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  return rle8mmtf_index_emit_enqueue(p, (uint8_t *)dOut, dOutSize, ws, spacing, (uint8_t *)dIndex, dIndexSize, st) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

int hsrle_rle8_mmtf128_index_build_dev_async(const void *dStream, uint64_t streamSize, uint64_t uncompressedSize, uint32_t spacingRows, void *dIndex, uint64_t indexCapacity,
                                             uint64_t *dIndexSize, uint32_t *dStatus, void *stream)
{
  const uint32_t spacing = rm_index_spacing(spacingRows);
  if (dStream == nullptr || dStatus == nullptr || streamSize == 0u || uncompressedSize == 0u || uncompressedSize > kRle8MmtfMaxIn || spacing == 0u ||
      !rm_index_args_ok(dIndex, dIndexSize) || !word_aligned(dStatus, 4) || ranges_overlap(dIndex, indexCapacity, dStream, streamSize))
    return HSRLE_ERR_ARGUMENT;
  if (indexCapacity < rm_index_bound(uncompressedSize, spacing))
    return HSRLE_ERR_CAPACITY;
  return rle8mmtf_index_build_enqueue((const uint8_t *)dStream, clamp32(streamSize), (uint32_t)uncompressedSize, spacing, (uint8_t *)dIndex, dIndexSize, dStatus,
                                      (hipStream_t)stream) == hipSuccess
           ? HSRLE_OK
           : HSRLE_ERR_DEVICE;
}

int hsrle_rle8_mmtf128_decompress_indexed_dev_async(const void *dStream, uint64_t streamSize, const void *dIndex, const hsrle_mono_index_info_t *info, void *dOut, uint64_t outSize,
                                                    uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize, void *stream)
{
  Rle8MmtfPlan p;
  const int rc = stream_decompress_check(rle8mmtf_dec_plan, dStream, streamSize, dOut, outSize, dStatus, dWorkspace, workspaceSize, p);
  if (rc == HSRLE_ERR_ARGUMENT || dIndex == nullptr || info == nullptr || !rm_index_info_ok(*info) || info->uncompressedSize != outSize ||
      ranges_overlap(dIndex, info->indexBytes, dOut, outSize))
    return HSRLE_ERR_ARGUMENT;
  if (rc != HSRLE_OK)
    return rc;
  return rle8mmtf_decompress_indexed_enqueue(p, (const uint8_t *)dStream, clamp32(streamSize), (const uint8_t *)dIndex, info->compressedSize, info->spacing, info->recordCount,
                                             (uint8_t *)dOut, dStatus, workspace_start(dWorkspace), (hipStream_t)stream) == hipSuccess
           ? HSRLE_OK
           : HSRLE_ERR_DEVICE;
}

// The two host-pointer calls: the staged trip.  Status word and index size word: Staging::status[0] and [2 .. 3].
int hsrle_rle8_mmtf128_index_build_host(const void *pStream, uint64_t streamSize, uint32_t spacingRows, void *pIndex, uint64_t indexCapacity, uint64_t *pIndexSize)
{
  if (pStream == nullptr || pIndex == nullptr || pIndexSize == nullptr || streamSize < 8u || streamSize > 0xFFFFFFFFull)
    return HSRLE_ERR_ARGUMENT;
  uint32_t hdr[2];
  memcpy(hdr, pStream, 8);
  const uint64_t bound = rm_index_bound(hdr[0], spacingRows);
  if (hdr[0] == 0u || bound == 0u)
    return rm_index_spacing(spacingRows) == 0u ? HSRLE_ERR_ARGUMENT : HSRLE_ERR_FORMAT;
  if (indexCapacity < bound)
    return HSRLE_ERR_CAPACITY;
  if (!device_ok())
    return HSRLE_ERR_DEVICE;
  return staged_call(
    pStream, streamSize, bound, 256u, pIndex, 4u,
    [&](Staging &s) { return hsrle_rle8_mmtf128_index_build_dev_async(s.in, streamSize, hdr[0], spacingRows, s.out, bound, (uint64_t *)(s.status + 2), s.status, nullptr); },
    [&](const uint32_t *h, uint64_t &n) { n = (uint64_t)h[2] | (uint64_t)h[3] << 32; return h[0] != HSRLE_RLE8_MMTF_DONE || n < 64u || n > bound ? HSRLE_ERR_FORMAT : HSRLE_OK; },
    pIndexSize);
}

int hsrle_rle8_mmtf128_decompress_indexed_host(const void *pStream, uint64_t streamSize, const void *pIndex, uint64_t indexSize, void *pOut, uint64_t outCapacity,
                                               uint64_t *pUncompressedSize)
{
  if (pStream == nullptr || pIndex == nullptr || pOut == nullptr || pUncompressedSize == nullptr || streamSize < 8u || streamSize > 0xFFFFFFFFull)
    return HSRLE_ERR_ARGUMENT;
  hsrle_mono_index_info_t info;
  const int rc = hsrle_rle8_mmtf128_index_info_host(pIndex, indexSize, &info);
  if (rc != HSRLE_OK)
    return rc;
  if (outCapacity < info.uncompressedSize)
    return HSRLE_ERR_CAPACITY;
  const uint64_t need = hsrle_rle8_mmtf128_workspace_size(1, info.uncompressedSize), indexAt = align_up(streamSize, 256);
  if (need == 0u || !device_ok())
    return HSRLE_ERR_DEVICE;
  return staged_call(
    pStream, streamSize, info.uncompressedSize, need, pOut, 1u,
    [&](Staging &s) {
      if (!s.up(pIndex, info.indexBytes, indexAt))
        return (int)HSRLE_ERR_DEVICE;
      return hsrle_rle8_mmtf128_decompress_indexed_dev_async(s.in, streamSize, s.in + indexAt, &info, s.out, info.uncompressedSize, s.status, s.ws, s.wsSize, nullptr);
    },
    [&](const uint32_t *h, uint64_t &n) { n = info.uncompressedSize; return h[0] != HSRLE_RLE8_MMTF_DONE ? HSRLE_ERR_FORMAT : HSRLE_OK; }, pUncompressedSize,
    indexAt - streamSize + info.indexBytes);
}

// ---- checkpoints and byte-range decode ----
uint64_t hsrle_rle8_mmtf128_checkpoints_bound(uint64_t uncompressedSize, uint32_t checkpointRows) { return rm_checkpoints_bound(uncompressedSize, checkpointRows); }

int hsrle_rle8_mmtf128_checkpoints_info_host(const void *pCheckpoints, uint64_t size, void *pInfo)
{
  if (pCheckpoints == nullptr || pInfo == nullptr)
    return HSRLE_ERR_ARGUMENT;
  uint32_t w[16];
  if (size < sizeof(w))
    return HSRLE_ERR_FORMAT;
  memcpy(w, pCheckpoints, sizeof(w));
  hsrle_rle8_mmtf128_checkpoints_info_t i = {};
  i.version = w[2]; i.headerBytes = w[3];
  i.uncompressedSize = w[4]; i.streamSize = w[5];
  i.checkpointRows = w[6]; i.checkpointCount = w[7];
  i.size = (uint64_t)w[8] | (uint64_t)w[9] << 32;
  bool zeros = true;
  for (int k = 10; k < 16; k++) zeros = zeros && w[k] == 0u;
  if (memcmp(w, "HSRLEMFC", 8) != 0 || !zeros || !rm_checkpoints_info_ok(i) || i.size > size)
    return HSRLE_ERR_FORMAT;
  *(hsrle_rle8_mmtf128_checkpoints_info_t *)pInfo = i;
  return HSRLE_OK;
}

int hsrle_rle8_mmtf128_checkpoints_build_dev_async(const void *dStream, uint64_t streamSize, const void *dIndex, const hsrle_mono_index_info_t *indexInfo, uint32_t checkpointRows,
                                                   void *dCheckpoints, uint64_t capacity, uint64_t *dSize, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize,
                                                   void *stream)
{
  const uint32_t rows = rm_checkpoint_rows(checkpointRows);
  Rle8MmtfPlan p;
  if (dStream == nullptr || dIndex == nullptr || indexInfo == nullptr || dCheckpoints == nullptr || dSize == nullptr || dStatus == nullptr || dWorkspace == nullptr ||
      streamSize == 0u || rows == 0u || !rm_index_info_ok(*indexInfo) || !rle8mmtf_dec_plan(indexInfo->uncompressedSize, p))
    return HSRLE_ERR_ARGUMENT;
  if (!word_aligned(dSize, 8) || !word_aligned(dStatus, 4) || ranges_overlap(dCheckpoints, capacity, dStream, streamSize) ||
      ranges_overlap(dCheckpoints, capacity, dIndex, indexInfo->indexBytes))
    return HSRLE_ERR_ARGUMENT;
  if (capacity < rm_checkpoints_bound(p.size, rows) || workspaceSize < p.total)
    return HSRLE_ERR_CAPACITY;
  return rle8mmtf_checkpoints_build_enqueue(p, (const uint8_t *)dStream, clamp32(streamSize), (const uint8_t *)dIndex, indexInfo->compressedSize, indexInfo->spacing,
                                            indexInfo->recordCount, rows, rm_checkpoint_count(p.size, rows), (uint8_t *)dCheckpoints, dSize, dStatus, workspace_start(dWorkspace),
                                            (hipStream_t)stream) == hipSuccess
           ? HSRLE_OK
           : HSRLE_ERR_DEVICE;
}

uint64_t hsrle_rle8_mmtf128_range_workspace_size(uint64_t length, uint32_t spacingRows, uint32_t checkpointRows)
{
  const uint32_t spacing = rm_index_spacing(spacingRows), rows = rm_checkpoint_rows(checkpointRows);
  RmRangePlan p;
  if (length == 0u || length > kRle8MmtfMaxIn || spacing == 0u || rows == 0u || !rm_range_layout(rm_range_max_rows(length, rows), 15u, spacing, p))
    return 0u;
  return p.total;
}

int hsrle_rle8_mmtf128_decompress_range_dev_async(const void *dStream, uint64_t streamSize, const void *dIndex, const hsrle_mono_index_info_t *indexInfo, const void *dCheckpoints,
                                                  const void *checkpointsInfo, uint64_t offset, uint64_t length, void *dOut, uint64_t outCapacity, uint32_t *dStatus,
                                                  void *dWorkspace, uint64_t workspaceSize, void *stream)
{
  const hsrle_rle8_mmtf128_checkpoints_info_t *ck = (const hsrle_rle8_mmtf128_checkpoints_info_t *)checkpointsInfo;
  if (dStream == nullptr || dIndex == nullptr || indexInfo == nullptr || dCheckpoints == nullptr || ck == nullptr || dOut == nullptr || dStatus == nullptr ||
      dWorkspace == nullptr || streamSize == 0u || !rm_index_info_ok(*indexInfo) || !rm_checkpoints_info_ok(*ck) || !word_aligned(dStatus, 4))
    return HSRLE_ERR_ARGUMENT;
  const uint64_t size = indexInfo->uncompressedSize;
  if (ck->uncompressedSize != size || ck->streamSize != indexInfo->compressedSize || offset > size || length > size - offset || outCapacity < length ||
      ranges_overlap(dOut, length, dStream, streamSize) || ranges_overlap(dOut, length, dIndex, indexInfo->indexBytes) || ranges_overlap(dOut, length, dCheckpoints, ck->size))
    return HSRLE_ERR_ARGUMENT;
  if (length == 0u)
    return HSRLE_OK;
  RmRangePlan p;
  if (!rm_range_plan(size, offset, length, indexInfo->spacing, ck->checkpointRows, p))
    return HSRLE_ERR_ARGUMENT;
  if (workspaceSize < p.total)
    return HSRLE_ERR_CAPACITY;
  return rle8mmtf_decompress_range_enqueue(p, (const uint8_t *)dStream, clamp32(streamSize), (const uint8_t *)dIndex, indexInfo->compressedSize, indexInfo->spacing,
                                           indexInfo->recordCount, (const uint8_t *)dCheckpoints, ck->checkpointRows, ck->checkpointCount, (uint8_t *)dOut, length, dStatus,
                                           workspace_start(dWorkspace), (hipStream_t)stream) == hipSuccess
           ? HSRLE_OK
           : HSRLE_ERR_DEVICE;
}

// The two host-pointer calls: the staged trip, the sidecars behind the stream in the input staging.  Status word and size word: Staging::status[0] and [2 .. 3].
int hsrle_rle8_mmtf128_checkpoints_build_host(const void *pStream, uint64_t streamSize, const void *pIndex, uint64_t indexSize, uint32_t checkpointRows, void *pCheckpoints,
                                              uint64_t capacity, uint64_t *pSize)
{
  if (pStream == nullptr || pIndex == nullptr || pCheckpoints == nullptr || pSize == nullptr || streamSize < 8u || streamSize > 0xFFFFFFFFull ||
      rm_checkpoint_rows(checkpointRows) == 0u)
    return HSRLE_ERR_ARGUMENT;
  hsrle_mono_index_info_t info;
  const int rc = hsrle_rle8_mmtf128_index_info_host(pIndex, indexSize, &info);
  if (rc != HSRLE_OK)
    return rc;
  const uint64_t bound = rm_checkpoints_bound(info.uncompressedSize, checkpointRows);
  if (capacity < bound)
    return HSRLE_ERR_CAPACITY;
  const uint64_t need = hsrle_rle8_mmtf128_workspace_size(1, info.uncompressedSize), indexAt = align_up(streamSize, 256);
  if (need == 0u || !device_ok())
    return HSRLE_ERR_DEVICE;
  return staged_call(
    pStream, streamSize, bound, need, pCheckpoints, 4u,
    [&](Staging &s) {
      if (!s.up(pIndex, info.indexBytes, indexAt))
        return (int)HSRLE_ERR_DEVICE;
      return hsrle_rle8_mmtf128_checkpoints_build_dev_async(s.in, streamSize, s.in + indexAt, &info, checkpointRows, s.out, bound, (uint64_t *)(s.status + 2), s.status, s.ws,
                                                            s.wsSize, nullptr);
    },
    [&](const uint32_t *h, uint64_t &n) { n = (uint64_t)h[2] | (uint64_t)h[3] << 32; return h[0] != HSRLE_RLE8_MMTF_DONE || n != bound ? HSRLE_ERR_FORMAT : HSRLE_OK; }, pSize,
    indexAt - streamSize + info.indexBytes);
}

int hsrle_rle8_mmtf128_decompress_range_host(const void *pStream, uint64_t streamSize, const void *pIndex, uint64_t indexSize, const void *pCheckpoints, uint64_t checkpointsSize,
                                             uint64_t offset, uint64_t length, void *pOut, uint64_t outCapacity)
{
  if (pStream == nullptr || pIndex == nullptr || pCheckpoints == nullptr || pOut == nullptr || streamSize < 8u || streamSize > 0xFFFFFFFFull)
    return HSRLE_ERR_ARGUMENT;
  hsrle_mono_index_info_t info;
  hsrle_rle8_mmtf128_checkpoints_info_t ck;
  int rc = hsrle_rle8_mmtf128_index_info_host(pIndex, indexSize, &info);
  if (rc == HSRLE_OK) rc = hsrle_rle8_mmtf128_checkpoints_info_host(pCheckpoints, checkpointsSize, &ck);
  if (rc != HSRLE_OK)
    return rc;
  if (ck.uncompressedSize != info.uncompressedSize || ck.streamSize != info.compressedSize || offset > info.uncompressedSize || length > info.uncompressedSize - offset ||
      outCapacity < length)
    return HSRLE_ERR_ARGUMENT;
  if (length == 0u)
    return HSRLE_OK;
  const uint64_t need = hsrle_rle8_mmtf128_range_workspace_size(length, info.spacing, ck.checkpointRows), indexAt = align_up(streamSize, 256),
                 ckAt = align_up(indexAt + info.indexBytes, 256);
  if (need == 0u || !device_ok())
    return HSRLE_ERR_DEVICE;
  uint64_t copied = 0;
  return staged_call(
    pStream, streamSize, length, need, pOut, 1u,
    [&](Staging &s) {
      if (!s.up(pIndex, info.indexBytes, indexAt) || !s.up(pCheckpoints, ck.size, ckAt))
        return (int)HSRLE_ERR_DEVICE;
      return hsrle_rle8_mmtf128_decompress_range_dev_async(s.in, streamSize, s.in + indexAt, &info, s.in + ckAt, &ck, offset, length, s.out, length, s.status, s.ws, s.wsSize,
                                                           nullptr);
    },
    [&](const uint32_t *h, uint64_t &n) { n = length; return h[0] != HSRLE_RLE8_MMTF_DONE ? HSRLE_ERR_FORMAT : HSRLE_OK; }, &copied, ckAt - streamSize + ck.size);
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
