// hsrle_capi_mono_encode.h -- part of hsrle_capi.hip: monolithic stream encode by many lanes (hsrle_mono_encode.hip.h): cut behind long runs, block kernels in MONO mode, compaction
#pragma once
#include "hsrle_capi_container.h"
#include "hsrle_capi_mono_decode.h"

namespace hsrle {

constexpr uint32_t kMonoListRounds = 64u;     // repair rounds of the guessed move-to-front lists before the caller falls back to one lane
__global__ void k_copy_word(const uint32_t *__restrict__ from, uint32_t *__restrict__ to) { *to = *from; }

static thread_local uint32_t g_monoEncLast[4] = { 0, 0, 0, 0 };   // this thread's last list-codec encode: extra rounds, chunks encoded again in rounds 1, 2, chunks the proof rejected (hsrle_mono_encode_stats)

struct MonoEncPlan
{
  uint32_t G, pieces;
  bool windowed;                                       // hsrle_codecs.h chunk_mode(): chunks of any length by the windowed position-parallel encoders (hsrle_encode8pw.hip.h, hsrle_encodeSpw.hip.h)
  uint64_t offCutPos, offCutSym, offFlags, offIdx, offStarts, offSyms, offSlotOff, offSizes, offOffsets, offCtrl, offSlots, total;
  ScanLevels levels;                                   // of the scans over the pieces' flags and the chunks' sizes (at most pieces + 2 values)
  uint64_t offGuess, offListOut, offRoll1, offRoll2;   // codecs with a move-to-front list: 8 words per chunk / per 64 / per 4096 chunks
  uint64_t offPick;                                    // 8 bit Single: the symbol pick's sums (k_single_pick_mono)
  uint64_t offJobs; uint32_t jobCap;                   // 8 bit Single: literal stretches noted by the chunk encoders for k_copy_jobs
};

// the codecs whose chunks have a windowed launcher (hsrle_capi_container.h: ppw_pick), unless an A/B build or HSRLE_PP=2 (read per call: tools/mono_encode_time.py) says never
static bool mono_windowed(int codec) { return ppw_pick(codec, true).launch != nullptr && kPpwMinBlocks != 0xFFFFFFFFu && knob_u32("HSRLE_PP", 0u) != 2u; }

static MonoEncPlan plan_mono_encode(uint32_t U, int codec, bool lists = true)
{
  MonoEncPlan m;
  init_tables();
  m.windowed = mono_windowed(codec);
  // ~131 072 pieces (= lanes) keep the device busy: 1 GiB: 8 KiB pieces 780 GiB/s, 4 KiB 720; 256 MiB: 2 KiB 523, 4 KiB 321; 88 MB: 1 KiB 286, 2 KiB 224
  uint32_t G = 1024u;
  while (G < 8192u && ((uint64_t)U + G - 1u) / G > 131072ull) G *= 2u;
  // windowed: a chunk is a WAVE's work and every chunk ends with a partial window, so the pieces are several windows long as soon as that leaves
  // ~6 000 of them (1 GiB: 4 / 8 / 16 / 32 / 64 / 128 KiB pieces 1.72 / 1.23 / 1.09 / 1.00 / 0.95 / 0.97 ms; 88 MB: 0.25 / 0.22 / 0.20 / 0.21 / 0.22 / 0.26)
  if (m.windowed) { G = 8192u; while (G < 65536u && (uint64_t)U / G > 6000ull) G *= 2u; }
  if (g_monoTune[1] >= 32u && g_monoTune[1] <= (1u << 24)) G = g_monoTune[1];
  m.G = G;
  m.pieces = (uint32_t)(((uint64_t)U + G - 1u) / G);
  const uint64_t n = m.pieces;
  uint64_t at = 0;
  m.offCutPos = at; at += align_up(8ull * n, 256);
  m.offCutSym = at; at += align_up(8ull * n, 256);
  m.offFlags = at; at += align_up(4ull * n, 256);
  m.offIdx = at; at += align_up(8ull * (n + 1), 256);
  m.offStarts = at; at += align_up(8ull * (n + 2), 256);
  m.offSyms = at; at += align_up(8ull * (n + 1), 256);
  m.offSlotOff = at; at += align_up(8ull * (n + 1), 256);
  m.offSizes = at; at += align_up(4ull * (n + 1), 256);
  m.offOffsets = at; at += align_up(8ull * (n + 2), 256);
  m.levels.lay_out(n + 2, at);
  m.offCtrl = at; at += 256;
  m.offPick = at; at += 4096;
  m.jobCap = U / 1024u + 16u;                                            // (every stretch of >= kCopyJobMin bytes there can be)
  m.offJobs = at; at += align_up(24ull * m.jobCap, 256);
  m.offGuess = m.offListOut = m.offRoll1 = m.offRoll2 = at;
  if (lists)
  {
    m.offGuess = at; at += align_up(64ull * (n + 1), 256);
    m.offListOut = at; at += align_up(64ull * (n + 1), 256);
    m.offRoll1 = at; at += align_up(64ull * ((n + 1) / 64 + 1), 256);
    m.offRoll2 = at; at += align_up(64ull * ((n + 1) / 4096 + 1), 256);
  }
  // (windowed: no staging slots -- the window states and records live there: 32 (8 bit) / 64 + 1 024 bytes per window, at most U / 4 096 + chunks windows)
  const uint64_t windowsMax = ((uint64_t)U >> 12) + n + 1ull;
  const uint64_t slotBytes = (uint64_t)U + ((uint64_t)U >> 7) + 256ull * (n + 2) + 4096ull;
  const uint64_t windowBytes = align_up(4ull * ppw_pick(codec, true).stateWords * windowsMax, 256) + 4ull * kPpwStride * windowsMax + 512ull;
  m.offSlots = at; at += align_up(m.windowed && windowBytes > slotBytes ? windowBytes : slotBytes, 256);
  m.total = at;
  return m;
}

// the enqueue-only encode's word for the caller (hsrle_compress_mono_dev_enqueue): the device-side twin of the synchronous checks behind the windowed encoders
// (ctrl[0] chunks, [2..3] the stream's size, [5] a chunk that did not end on its boundary run)
__global__ void k_mono_enc_status(const uint32_t *__restrict__ ctrl, uint32_t maxChunks, uint32_t *__restrict__ status, uint32_t *__restrict__ size)
{
  if (threadIdx.x != 0u) return;
  const uint32_t chunks = ctrl[0], lo = ctrl[2], hi = ctrl[3], fail = ctrl[5];
  const bool ok = chunks != 0u && chunks <= maxChunks && lo != 0u && hi == 0u && fail == 0u;
  *status = ok ? (uint32_t)HSRLE_MONO_DONE : (uint32_t)HSRLE_MONO_ENCODE_FAILED;
  if (size) *size = ok ? lo : 0u;
}

// dOut: capacity >= rle_compress_bounds(U).  Synchronises the stream twice (chunk count, stream size) -- the windowed encoders once, at the end.
// pSize == nullptr: the windowed encoders only, nothing synchronises; pChunks is then a DEVICE word for the stream's size, and dStatus (device, if not nullptr)
// receives HSRLE_MONO_DONE / HSRLE_MONO_ENCODE_FAILED (the size word then says 0 on failure).
static int mono_encode_dev(int codec, const uint8_t *dIn, uint32_t U, uint8_t *dOut, uint8_t *ws, const MonoEncPlan &m, uint32_t *pSize, uint32_t *pChunks, hipStream_t st,
                           uint32_t *dStatus = nullptr)
{
  init_tables();
  const CodecInfo &ci = kCodecs[codec];
  const int S = ci.S, listK = list_len(ci);
  const uint32_t longc = cut_long(ci);
  if (!g_launch[codec].menc)
    return HSRLE_ERR_UNSUPPORTED;
  const bool single = is_single(ci);
  const uint32_t hs = header_size(ci) + (single ? 1u : 0u);   // (Single: the symbol byte follows the header)
  uint64_t *cutPos = (uint64_t *)(ws + m.offCutPos), *idx = (uint64_t *)(ws + m.offIdx), *starts = (uint64_t *)(ws + m.offStarts), *slotOff = (uint64_t *)(ws + m.offSlotOff);
  uint64_t *offsets = (uint64_t *)(ws + m.offOffsets);
  uint64_t *cutSym = (uint64_t *)(ws + m.offCutSym), *syms = (uint64_t *)(ws + m.offSyms);
  uint32_t *flags = (uint32_t *)(ws + m.offFlags), *sizes = (uint32_t *)(ws + m.offSizes), *ctrl = (uint32_t *)(ws + m.offCtrl);
  const ScanLevels &w = m.levels;

  if (zero_async(ctrl, 64, st) != hipSuccess)                            // (a kernel, not hipMemsetAsync: the windowed flow below can be captured in a HIP graph, see zero_async)
    return HSRLE_ERR_DEVICE;
  if (single)
  {
    // the stream's ONE symbol first (rle8_extreme_cpu.c:53-153 over the whole input): sums per piece, then the estimator's end game and the argmax -> ctrl[8]
    uint32_t *table = (uint32_t *)(ws + m.offPick);
    const uint32_t pp = (U + kPickPiece - 1u) / kPickPiece;
    if (hipMemsetAsync(table, 0, 2064, st) != hipSuccess || hipMemsetAsync(table + 514, 0xFF, 8, st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
    hipLaunchKernelGGL(k_single_pick_mono, dim3(pp < 4096u ? pp : 4096u), dim3(64), 0, st, dIn, U, pp, table);
    hipLaunchKernelGGL(k_single_pick_final, dim3(1), dim3(64), 0, st, dIn, U, table, ctrl + 8);
  }
  const dim3 cgrid((m.pieces + 63u) / 64u);
  launch_cuts(S, ci.aligned, single ? (const uint32_t *)(ctrl + 8) : (const uint32_t *)nullptr, cgrid, st, dIn, (uint64_t)U, m.G, m.pieces, longc, cutPos, cutSym, flags);
  if (scan_sizes(flags, m.pieces, idx, ws, w, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  hipLaunchKernelGGL(k_mono_scatter, dim3((m.pieces + 255u) / 256u), dim3(256), 0, st, (const uint64_t *)cutPos, (const uint64_t *)cutSym, (const uint32_t *)flags, (const uint64_t *)idx,
                     m.pieces, (uint64_t)U, starts, syms, slotOff, ctrl);
  // the codecs whose state at a cut the cut fixes: the windowed position-parallel encoders take chunks of any length (hsrle_encode8pw.hip.h: rle8_multi /
  // rle8_packed_multi; hsrle_encodeSpw.hip.h in its chunk mode: plain / Packed / Short with no list or a one-symbol list) -- no step bound, no staging slots, no lists
  const uint64_t windowsMax = ((uint64_t)U >> 12) + m.pieces + 1ull;
  const bool windowed = m.windowed && mono_windowed(codec);
  if (windowed)
  {
    // every piece may be a chunk: a wave per possible chunk (those behind the last one write a zero size), a wave per possible window -- nothing is read back
    // before the end
    const PpwPick pick = ppw_pick(codec, true);
    PpwArgs pa{};
    pa.in = dIn; pa.U = U; pa.B = 0u; pa.nUnits = m.pieces + 1u; pa.starts = starts; pa.syms = syms; pa.count = ctrl; pa.sizes = sizes; pa.offsets = offsets; pa.payload = dOut + hs;
    ppw_lay_out(pa, ws + m.offSlots, pick.stateWords, windowsMax);
    pa.fail = ctrl + 5;                                                   // (zeroed above)
    g_monoEncLast[0] = g_monoEncLast[1] = g_monoEncLast[2] = g_monoEncLast[3] = 0u;   // (no list, no rounds)
    if (pick.launch(pa, 0, st) != hipSuccess || scan_sizes(sizes, pa.nUnits, offsets, ws, w, st) != hipSuccess || pick.launch(pa, 1, st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
    hipLaunchKernelGGL(k_mono_finish, dim3(1), dim3(64), 0, st, dOut, U, hs, (const uint64_t *)offsets, (const uint32_t *)ctrl, ctrl, 0u);
    if (pSize == nullptr)
    {
      // enqueue only: the size stays on the device (the stream's own header holds it; pChunks, if given, is a DEVICE word that receives it too)
      if (dStatus) hipLaunchKernelGGL(k_mono_enc_status, dim3(1), dim3(64), 0, st, (const uint32_t *)ctrl, m.pieces + 1u, dStatus, pChunks);
      else if (pChunks) hipLaunchKernelGGL(k_copy_word, dim3(1), dim3(1), 0, st, (const uint32_t *)(ctrl + 2), pChunks);
      return hipGetLastError() == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
    }
    uint32_t back[6] = { 0, 0, 0, 0, 0, 0 };                              // chunks, -, stream size (2 words), -, a chunk that missed its boundary run
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(back, ctrl, 24, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
    if (back[5] != 0u)
      return HSRLE_ERR_UNSUPPORTED;                                      // (never a stream with a hole: the drop-in functions then use one lane)
    if (back[0] == 0u || back[0] > m.pieces + 1u || back[3] != 0u || back[2] == 0u)
      return HSRLE_ERR_DEVICE;
    if (pChunks) *pChunks = back[0];
    *pSize = back[2];
    return HSRLE_OK;
  }
  hipLaunchKernelGGL(k_mono_longest, dim3((m.pieces + 1u + 255u) / 256u), dim3(256), 0, st, (const uint64_t *)starts, ctrl);
  uint32_t head[10] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
  if (hipMemcpyAsync(head, ctrl, 40, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  if (single && head[9] != 0u)
    return HSRLE_ERR_UNSUPPORTED;                                        // (a run of more than 16 MiB: the pick gave up -- callers fall back to one lane)
  const uint32_t chunks = head[0], longest = head[1];
  if (chunks == 0u || chunks > m.pieces + 1u)
    return HSRLE_ERR_DEVICE;
  if (pChunks) *pChunks = chunks;

  EncodeArgs ea{ dIn, (uint64_t)U, 0u, chunks, ws + m.offSlots, 0u, sizes };
  MonoEncodeArgs ma{ starts, syms, slotOff, 2u * (longest / 64u) + 64u };
  ma.pick = ctrl + 8;
  if (single) { ma.jobs = (uint64_t *)(ws + m.offJobs); ma.jobCount = ctrl + 12; ma.jobCap = m.jobCap; }   // (ctrl[12] was zeroed with the rest)
  if (listK == 0)
  {
    if (g_launch[codec].menc(ea, ma, st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
  }
  else
  {
    // move-to-front list: dry pass -> guessed lists -> encode -> verify, repeat for the chunks whose guess was wrong (hsrle_mono_encode.hip.h)
    uint64_t *guess = (uint64_t *)(ws + m.offGuess), *listOut = (uint64_t *)(ws + m.offListOut), *roll1 = (uint64_t *)(ws + m.offRoll1), *roll2 = (uint64_t *)(ws + m.offRoll2);
    const uint32_t n1 = (chunks + 63u) / 64u, n2 = (n1 + 63u) / 64u;
    ma.syms = guess; ma.listOut = listOut;
    hipLaunchKernelGGL(k_mono_list_default, dim3((chunks + 255u) / 256u), dim3(256), 0, st, chunks, (uint32_t)listK, (uint32_t)S, guess);
    ma.dry = 1u;
    if (g_launch[codec].menc(ea, ma, st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
    ma.dry = 0u;
    uint32_t rounds = 0;
    g_monoEncLast[0] = g_monoEncLast[1] = g_monoEncLast[2] = g_monoEncLast[3] = 0u;
    for (;; rounds++)
    {
      // lists from what the chunks did in the last pass; chunks whose list changed (first time: all) are encoded from it
      if (rounds > kMonoListRounds)
        return HSRLE_ERR_UNSUPPORTED;                                    // (callers fall back to one lane)
      if (hipMemsetAsync(ctrl + 4, 0, 4, st) != hipSuccess)
        return HSRLE_ERR_DEVICE;
      hipLaunchKernelGGL(k_mono_list_tiles, dim3((n1 + 63u) / 64u), dim3(64), 0, st, (const uint64_t *)listOut, chunks, (uint32_t)listK, roll1);
      hipLaunchKernelGGL(k_mono_list_tiles, dim3((n2 + 63u) / 64u), dim3(64), 0, st, (const uint64_t *)roll1, n1, (uint32_t)listK, roll2);
      hipLaunchKernelGGL(k_mono_list_guess, dim3((chunks + 63u) / 64u), dim3(64), 0, st, (const uint64_t *)listOut, (const uint64_t *)roll1, (const uint64_t *)roll2, chunks,
                         (uint32_t)listK, (uint32_t)S, guess, rounds == 0u ? 1u : 0u, ctrl + 4);
      if (rounds > 0u)
      {
        uint32_t todo = 0;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&todo, ctrl + 4, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
          return HSRLE_ERR_DEVICE;
        g_monoEncLast[0] = rounds - 1u;
        if (rounds <= 2u) g_monoEncLast[rounds] = todo;
        if (todo == 0u)
          break;
      }
      if (g_launch[codec].menc(ea, ma, st) != hipSuccess)
        return HSRLE_ERR_DEVICE;
    }
    for (;; rounds++)
    {
      // the proof (and, should the fixed point above not be one, the repair)
      if (hipMemsetAsync(ctrl + 4, 0, 4, st) != hipSuccess)
        return HSRLE_ERR_DEVICE;
      hipLaunchKernelGGL(k_mono_list_verify, dim3((chunks + 255u) / 256u), dim3(256), 0, st, guess, (const uint64_t *)listOut, chunks, (uint32_t)listK, ctrl + 4);
      uint32_t bad = 0;
      if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, ctrl + 4, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return HSRLE_ERR_DEVICE;
      g_monoEncLast[3] += bad;
      if (bad == 0u)
        break;
      if (rounds > kMonoListRounds)
        return HSRLE_ERR_UNSUPPORTED;
      if (g_launch[codec].menc(ea, ma, st) != hipSuccess)
        return HSRLE_ERR_DEVICE;
    }
  }
  if (scan_sizes(sizes, chunks, offsets, ws, w, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  launch_compact_var(false, (const uint8_t *)(ws + m.offSlots), (const uint64_t *)slotOff, (const uint64_t *)offsets, dOut + hs, chunks, st);
  if (single || ci.greedy)
    hipLaunchKernelGGL(k_mono_zero_sizes, dim3((chunks + 255u) / 256u), dim3(256), 0, st, (const uint32_t *)sizes, chunks, ctrl + 5);
  hipLaunchKernelGGL(k_mono_finish, dim3(1), dim3(64), 0, st, dOut, U, hs, (const uint64_t *)offsets, (const uint32_t *)ctrl, ctrl, ci.fam == SHORT_SINGLE ? 1u : 0u);
  uint32_t tail[4] = { 0, 0, 0, 0 };
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tail, ctrl + 2, 16, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  if (tail[3] != 0u)
    return HSRLE_ERR_UNSUPPORTED;                                        // (a Single chunk that did not end on its boundary run: one lane, by the caller)
  if (tail[1] != 0u || tail[0] == 0u)
    return HSRLE_ERR_DEVICE;
  *pSize = tail[0];
  return HSRLE_OK;
}

} // namespace hsrle
