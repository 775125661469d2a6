// hsrle_capi_low_entropy.h -- part of hsrle_capi.hip: rle8m and the unsectioned low-entropy codec on device pointers (host-pointer forms: hsrle_capi_dropin.h)
#pragma once
#include "hsrle_capi_kernels.h"
#include "hsrle_rle8m.hip.h"

namespace hsrle {

// ---- rle8m: the reference's GPU decode path, rle8m_opencl_decompress (src/rle8_ocl.c:265-413) ----

constexpr uint32_t kRle8mWaveBelow = 131072u;   // measured on 1 GiB: 65 536 sections 570 (wave) against 321 GiB/s (lane), 262 144 sections 344-498 against 612-680

static int rle8m_decode_async(const void *dStream, uint64_t streamSize, uint32_t uncompressedSize, uint32_t sections, void *dOut, uint64_t outCapacity,
                              uint32_t *dStatus, hipStream_t st)
{
  // the caller has checked device_ok()
  if (!dStream || !dOut || streamSize < 12 || sections == 0 || uncompressedSize == 0 || outCapacity < uncompressedSize)
    return HSRLE_ERR_ARGUMENT;
  if (dStatus && zero_async(dStatus, 4, st) != hipSuccess)               // (a kernel, not hipMemsetAsync: graph capturable, see zero_async)
    return HSRLE_ERR_DEVICE;
  // few, large sections: one wave per section (one lane per section needs ~1e5 sections to fill the GPU)
  static const int forced = (int)knob_u32("HSRLE_RLE8M_DECODE", 0);   // 1 = lane, 2 = wave kernel (A/B runs)
  // ... and sections of 4 KiB and more decode faster that way whatever their number (1 GiB, 4 KiB sections: 1034 against 717 GiB/s on
  // video-shaped bytes, 618 against 629 on bytes that do not compress; 1 KiB sections: 841 / 501 against 737 / 617)
  const bool wave = forced ? forced == 2 : (sections < kRle8mWaveBelow || uncompressedSize / sections >= 4096u);
  if (wave)
    hipLaunchKernelGGL(k_rle8m_decode_wave, dim3(sections), dim3(64), 0, st, (const uint8_t *)dStream, streamSize, (uint8_t *)dOut, dStatus, uncompressedSize, sections);
  else
    hipLaunchKernelGGL(k_rle8m_decode, dim3((sections + 63u) / 64u), dim3(64), 0, st, (const uint8_t *)dStream, streamSize, (uint8_t *)dOut, dStatus, uncompressedSize, sections);
  return hipGetLastError() == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

// rle8m encode (device resident): workspace = [Rle8mTables][offsets u64 x (sections + 1)][statistics][slots][sizes u32][scan levels]
// (launch_le_stats below: three words per 4 KiB of input)
static inline uint64_t le_stats_ws_bytes(uint64_t n) { return 3ull * align_up(4ull * ((n + 4095ull) / 4096ull + 1ull), 256); }
struct Rle8mPlan
{
  ScanLevels levels;             // of the scan over the sections' sizes
  uint64_t offTables, offOffsets, offStats, offSlots, offSizes, total;
  uint32_t slotStride;
};

static Rle8mPlan plan_rle8m(uint32_t n, uint32_t sections)
{
  Rle8mPlan p;
  const uint32_t ss = n / sections, lastLen = n - ss * (sections - 1u);
  p.slotStride = (uint32_t)align_up(2ull * (uint64_t)(lastLen > ss ? lastLen : ss) + 16ull, 16);   // a section grows to at most twice its size
  uint64_t at = 0;
  p.offTables = at; at += align_up(sizeof(Rle8mTables), 256);
  p.offOffsets = at; at += align_up(((uint64_t)sections + 1ull) * 8ull, 256);
  p.offStats = at; at += le_stats_ws_bytes(n);
  p.offSlots = at; at += align_up((uint64_t)sections * p.slotStride, 256);
  p.offSizes = at; at += align_up((uint64_t)sections * 4ull, 256);
  p.levels.lay_out(sections, at);
  p.total = at;
  return p;
}

// the statistics of the low-entropy encoders (rle8_low_entropy_cpu.c:264-296) over the whole input: k_rle8m_stats_wave piece by piece, the pieces' run starts
// scanned, the token boundaries of runs that cross pieces added (hsrle_rle8m.hip.h, round 6: no lane follows a run through global memory any more).
// wsStats: le_stats_ws_bytes(n) bytes; *pRunStart4 (optional): the start of the run that covers the first byte of every 4 KiB piece (k_le_cuts)
static hipError_t launch_le_stats(const uint8_t *dIn, uint32_t n, Rle8mTables *t, uint32_t maxLen, uint8_t *wsStats, hipStream_t st, uint32_t maxWaves = 32768u, const uint32_t **pRunStart4 = nullptr)
{
  const uint32_t p4 = (uint32_t)(((uint64_t)n + 4095u) / 4096u);
  const uint64_t stride = align_up(4ull * ((uint64_t)p4 + 1ull), 256);
  uint32_t *lastB4 = (uint32_t *)wsStats, *firstB4 = (uint32_t *)(wsStats + stride), *runStart4 = (uint32_t *)(wsStats + 2ull * stride);
  uint32_t grid = p4 < maxWaves ? p4 : maxWaves;
  if ((uint64_t)grid * kRle8mStatsPieces < p4) grid = (p4 + kRle8mStatsPieces - 1u) / kRle8mStatsPieces;   // (no wave gets more pieces than its packed counters hold)
  hipLaunchKernelGGL(k_rle8m_stats_wave, dim3(grid), dim3(64), 0, st, dIn, n, t, maxLen, lastB4, firstB4);
  hipLaunchKernelGGL(k_le_scan_last, dim3(1), dim3(1024), 0, st, (const uint32_t *)lastB4, p4, runStart4);
  hipLaunchKernelGGL(k_le_stats_fixup, dim3((p4 + 255u) / 256u), dim3(256), 0, st, dIn, n, p4, (const uint32_t *)lastB4, (const uint32_t *)firstB4, (const uint32_t *)runStart4, t, maxLen);
  if (pRunStart4) *pRunStart4 = runStart4;
  return hipGetLastError();
}

static uint32_t rle8m_bounds(uint32_t sections, uint32_t n) { return n + (256 / 8) + 1 + 256 + 4u * (2u + sections - 1u + 1u); }

// The encoders keep words in their workspace -- counters that take atomics, 64-bit offsets -- at multiples of 256 bytes from its start, and zero the status
// word with a word store: a workspace or a status word at an odd address is refused on the host (input and output may start at any byte).
static inline bool encode_words_aligned(const void *dWs, const uint32_t *dStatus) { return ((uintptr_t)dWs & 15u) == 0u && ((uintptr_t)dStatus & 3u) == 0u; }

// the caller has checked device_ok()
// maxLen / onlyMax: the four unsectioned encoders share these kernels (rle8_low_entropy[_short]_compress[_only_max_frequency]: runs are cut
// every 255 or 32 bytes, and either every symbol whose runs average >= 2 carries repeat codes or only the one that saves the most)
static int rle8m_encode_async(const void *dIn, uint32_t n, uint32_t sections, void *dOut, uint64_t outCapacity, void *dWs, uint64_t wsSize, uint32_t *dStatus, hipStream_t st,
                              uint32_t maxLen = 255u, uint32_t onlyMax = 0u)
{
  if (!dIn || !dOut || !dWs || n == 0 || sections == 0 || !encode_words_aligned(dWs, dStatus))
    return HSRLE_ERR_ARGUMENT;
  if (outCapacity < rle8m_bounds(sections, n))
    return HSRLE_ERR_CAPACITY;
  const Rle8mPlan p = plan_rle8m(n, sections);
  if (wsSize < p.total)
    return HSRLE_ERR_CAPACITY;
  uint8_t *ws = (uint8_t *)dWs;
  Rle8mTables *t = (Rle8mTables *)(ws + p.offTables);
  uint64_t *offsets = (uint64_t *)(ws + p.offOffsets);
  uint32_t *sizes = (uint32_t *)(ws + p.offSizes);
  if (zero_async(t, sizeof(Rle8mTables), st) != hipSuccess || (dStatus && zero_async(dStatus, 4, st) != hipSuccess))
    return HSRLE_ERR_DEVICE;
  const uint32_t grid = (sections + 63u) / 64u;
  // the statistics are over the whole input: one lane per 4 KiB piece, whatever the section count
  const uint32_t pieces = (n / 4096u > sections) ? n / 4096u : sections;
  static const uint32_t g_rle8mStatsWaves = knob_u32("HSRLE_RLE8M_STATS_WAVES", 32768u);   // (1 GiB run-distributed / video-shaped: 1 024 waves 7.5 / 6.2 ms per encode, 8 192: 3.96 / 4.17, 32 768: 3.75 / 3.98; the byte-walking kernel: 4.03 / 4.60)
  static const int statsV1 = (int)knob_u32("HSRLE_RLE8M_STATS", 0);   // 1 = the byte-walking kernel (A/B runs)
  if (statsV1 == 1)
    hipLaunchKernelGGL(k_rle8m_stats, dim3((pieces + 63u) / 64u), dim3(64), 0, st, (const uint8_t *)dIn, n, pieces, t, maxLen);
  else
  {
    if (launch_le_stats((const uint8_t *)dIn, n, t, maxLen, ws + p.offStats, st, g_rle8mStatsWaves) != hipSuccess)
      return HSRLE_ERR_DEVICE;
  }
  hipLaunchKernelGGL(k_rle8m_info, dim3(1), dim3(256), 0, st, t, sections, (uint8_t *)dOut, onlyMax);
  static const int forced = (int)knob_u32("HSRLE_RLE8M_ENCODE", 0);   // 1 = lane, 2 = wave kernel (A/B runs)
  if (forced ? forced == 2 : sections < kRle8mWaveBelow)
    hipLaunchKernelGGL(k_rle8m_encode_wave, dim3(sections), dim3(64), 0, st, (const uint8_t *)dIn, n, sections, (const Rle8mTables *)t, ws + p.offSlots, p.slotStride, sizes, maxLen);
  else
    hipLaunchKernelGGL(k_rle8m_encode, dim3(grid), dim3(64), 0, st, (const uint8_t *)dIn, n, sections, (const Rle8mTables *)t, ws + p.offSlots, p.slotStride, sizes, maxLen);
  if (scan_sizes(sizes, sections, offsets, ws, p.levels, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  hipLaunchKernelGGL(k_rle8m_place, dim3((sections + 3u) / 4u), dim3(256), 0, st, (const uint8_t *)(ws + p.offSlots), p.slotStride, (const uint64_t *)offsets, (const Rle8mTables *)t,
                     (uint8_t *)dOut, outCapacity, n, sections, dStatus);
  return hipGetLastError() == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

// ---- the low-entropy codec in its UNSECTIONED forms (src/rle.h:53-57, :90-93; rle8_low_entropy_cpu.c:6-124, rle8_low_entropy_short_cpu.c:16-124):
//      [u32 compressedSize][u32 uncompressedSize][info][one stream].  Many waves on the one stream: the input is cut at run boundaries, the stream
//      at arbitrary bytes whose symbol / code parity a short backward scan finds (hsrle_rle8m.hip.h, "the UNSECTIONED low-entropy streams"). ----
static uint32_t le_bounds(uint32_t n) { return n + (256 / 8) + 1 + 256 + 8u; }

// many waves for ONE stream (hsrle_rle8m.hip.h, "the UNSECTIONED low-entropy streams"): pieces of kLePiece input / stream bytes
constexpr uint32_t kLePiece = 16384u;
struct LePlan
{
  ScanLevels levels;             // of the scan over the piece sizes
  uint32_t pieces;
  uint64_t offTables, offTmpTables, offTmpInfo, offCuts, offStats, offSizes, offOffsets, offSlots, total;
};
static LePlan plan_le(uint64_t bytes, bool withSlots, uint32_t piece = kLePiece)
{
  LePlan p;
  p.pieces = (uint32_t)((bytes + piece - 1u) / piece);
  if (p.pieces == 0u) p.pieces = 1u;
  uint64_t at = 0;
  p.offTables = at; at += align_up(sizeof(Rle8mTables), 256);
  p.offTmpTables = at; at += align_up(sizeof(Rle8mTables), 256);   // (le_compress_with_info: the statistics pass that only feeds the cut finder)
  p.offTmpInfo = at; at += 512;
  p.offCuts = at; at += align_up(4ull * ((uint64_t)p.pieces + 1ull), 256);
  p.offStats = at; at += le_stats_ws_bytes(bytes);                      // per 4 KiB of input: last / first run start, and the start of the run that enters (launch_le_stats)
  p.offSizes = at; at += align_up(4ull * ((uint64_t)p.pieces + 1ull), 256);
  p.offOffsets = at; at += align_up(8ull * ((uint64_t)p.pieces + 2ull), 256);
  p.levels.lay_out(p.pieces, at);
  p.offSlots = at; if (withSlots) at += align_up(2ull * bytes + 64ull, 256);
  p.total = at;
  return p;
}

// The body of an unsectioned encode for the tables in `t`: cuts -> a wave per piece -> size scan -> placement behind the header in dOut.
// runStart4: launch_le_stats' run starts of this input (whoever's tables that pass filled).  Only enqueues.
static int le_encode_pieces(const uint8_t *dIn, uint32_t n, const Rle8mTables *t, const uint32_t *runStart4, uint32_t maxLen, uint8_t *dOut, uint64_t outCapacity, uint8_t *ws, const LePlan &p,
                            uint32_t *dStatus, hipStream_t st)
{
  uint32_t *cuts = (uint32_t *)(ws + p.offCuts), *sizes = (uint32_t *)(ws + p.offSizes);
  uint64_t *offsets = (uint64_t *)(ws + p.offOffsets);
  hipLaunchKernelGGL(k_le_cuts, dim3((p.pieces + 63u) / 64u), dim3(64), 0, st, dIn, n, kLePiece, p.pieces, runStart4, t, maxLen, cuts);
  hipLaunchKernelGGL(k_le_encode_wave, dim3(p.pieces), dim3(64), 0, st, dIn, n, (const uint32_t *)cuts, p.pieces, t, ws + p.offSlots, sizes, maxLen);
  if (scan_sizes(sizes, p.pieces, offsets, ws, p.levels, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  hipLaunchKernelGGL(k_le_place, dim3((p.pieces + 3u) / 4u), dim3(256), 0, st, (const uint8_t *)(ws + p.offSlots), (const uint32_t *)cuts, (const uint64_t *)offsets, t, dOut, outCapacity, n, p.pieces, dStatus);
  return hipGetLastError() == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

// dOut: capacity >= le_bounds(n) (a stream that does not fit sets RLE8M_ERR_STREAM in *dStatus: the reference would write behind its
// caller's buffer there, rle8_low_entropy_cpu.c:476).  Only enqueues.  The stream's size is its first u32.
static int le_encode_async(const void *dIn, uint32_t n, void *dOut, uint64_t outCapacity, void *dWs, uint64_t wsSize, uint32_t *dStatus, uint32_t maxLen, uint32_t onlyMax, hipStream_t st)
{
  if (!dIn || !dOut || !dWs || n == 0 || !encode_words_aligned(dWs, dStatus))
    return HSRLE_ERR_ARGUMENT;
  if (outCapacity < le_bounds(n))
    return HSRLE_ERR_CAPACITY;
  const LePlan p = plan_le(n, true);
  if (wsSize < p.total)
    return HSRLE_ERR_CAPACITY;
  uint8_t *ws = (uint8_t *)dWs;
  Rle8mTables *t = (Rle8mTables *)(ws + p.offTables);
  if (zero_async(t, sizeof(Rle8mTables), st) != hipSuccess || (dStatus && zero_async(dStatus, 4, st) != hipSuccess))   // (ONE word: include/hsrle.h)
    return HSRLE_ERR_DEVICE;
  const uint32_t *runStart4 = nullptr;
  if (launch_le_stats((const uint8_t *)dIn, n, t, maxLen, ws + p.offStats, st, 32768u, &runStart4) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  hipLaunchKernelGGL(k_rle8m_info, dim3(1), dim3(256), 0, st, t, 1u, ws + p.offTmpInfo, onlyMax);
  hipLaunchKernelGGL(k_le_move_info, dim3(1), dim3(64), 0, st, (const uint8_t *)(ws + p.offTmpInfo), (const Rle8mTables *)t, (uint8_t *)dOut);
  return le_encode_pieces((const uint8_t *)dIn, n, t, runStart4, maxLen, (uint8_t *)dOut, outCapacity, ws, p, dStatus, st);
}

// dStream: the stream (nothing at or beyond streamSize is read), dataStart = 8 + 33 + listed symbols (the caller has read the header).  dStatus: three
// words ([0] error bits, [1] "a piece's parity could not be found within kLeCarryLimit bytes", [2] 1, or 2 with onePiece).  onePiece: decode with ONE wave (the fallback).
static int le_decode_async(const void *dStream, uint32_t streamSize, uint32_t dataStart, uint32_t expOut, void *dOut, uint64_t outCapacity, void *dWs, uint64_t wsSize, uint32_t *dStatus,
                           bool onePiece, hipStream_t st)
{
  if (!dStream || !dOut || !dWs || streamSize < dataStart || expOut == 0 || outCapacity < expOut || !dStatus)
    return HSRLE_ERR_ARGUMENT;
  const uint32_t body = streamSize - dataStart;
  const uint32_t G = onePiece ? (((body + 63u) / 64u) * 64u + 64u) : kLePiece;
  const LePlan p = plan_le(body, false, G);
  if (wsSize < p.total)
    return HSRLE_ERR_CAPACITY;
  uint8_t *ws = (uint8_t *)dWs;
  uint32_t *carry = (uint32_t *)(ws + p.offCuts), *sizes = (uint32_t *)(ws + p.offSizes);
  uint64_t *outStart = (uint64_t *)(ws + p.offOffsets);
  if (zero_async(dStatus, 8, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  hipLaunchKernelGGL(k_le_carry, dim3((p.pieces + 63u) / 64u), dim3(64), 0, st, (const uint8_t *)dStream, (uint64_t)streamSize, G, p.pieces, carry, dStatus, onePiece ? 2u : 1u);
  hipLaunchKernelGGL(k_le_decode_wave<true>, dim3(p.pieces), dim3(64), 0, st, (const uint8_t *)dStream, (uint64_t)streamSize, (uint8_t *)dOut, dStatus, expOut, G, p.pieces,
                     (const uint32_t *)carry, (const uint64_t *)nullptr, sizes);
  if (scan_sizes(sizes, p.pieces, outStart, ws, p.levels, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  hipLaunchKernelGGL(k_le_decode_wave<false>, dim3(p.pieces), dim3(64), 0, st, (const uint8_t *)dStream, (uint64_t)streamSize, (uint8_t *)dOut, dStatus, expOut, G, p.pieces,
                     (const uint32_t *)carry, (const uint64_t *)outStart, (uint32_t *)nullptr);
  return hipGetLastError() == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

// le_decode_async with its fallback and the verdict: many waves, then -- status[1]: a degenerate stretch of flagged-valued bytes -- once more with one wave.
// Reads the two status words behind each attempt (synchronises st).  HSRLE_OK / HSRLE_ERR_FORMAT / what le_decode_async returns.
static int le_decode_attempts(const void *dStream, uint32_t streamSize, uint32_t dataStart, uint32_t expOut, void *dOut, uint64_t outCapacity, void *dWs, uint64_t wsSize, uint32_t *dStatus,
                              hipStream_t st)
{
  uint32_t status[2] = { 1, 0 };
  for (int attempt = 0; attempt < 2; attempt++)
  {
    const int rc = le_decode_async(dStream, streamSize, dataStart, expOut, dOut, outCapacity, dWs, wsSize, dStatus, attempt != 0, st);
    if (rc != HSRLE_OK) return rc;
    if (hipMemcpyAsync(status, dStatus, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return HSRLE_ERR_DEVICE;
    if (status[1] == 0u) break;
  }
  return (status[0] != 0u || status[1] != 0u) ? HSRLE_ERR_FORMAT : HSRLE_OK;
}

} // namespace hsrle
