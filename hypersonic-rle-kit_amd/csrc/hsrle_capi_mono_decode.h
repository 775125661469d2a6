// hsrle_capi_mono_decode.h -- part of hsrle_capi.hip: monolithic stream decode -- index passes (hsrle_index.hip.h) + the block kernel started from entry records
#pragma once
#include "hsrle_capi_host.h"
#include "hsrle_index.hip.h"

namespace hsrle {

struct MonoPlan
{
  uint32_t G, M, B, R, KE;
  uint64_t nb;
  uint64_t offG, offE, offOlen, offT, offEntry, offOutStart, offStateIn, offFix, offList, offMark, offCtrl, offRec, offFast, offBatch, total;
  bool range7;
};

// (atomics: hsrle_mono_tuning() is a TEST knob and process-global -- a call that changes it between another thread's *_workspace_size() and
//  *_mono_dev() can make that workspace too small, which that call reports as HSRLE_ERR_CAPACITY; include/hsrle.h says so)
static std::atomic<uint32_t> g_monoTune[3] = { { env_u32("HSRLE_MONO_BLOCK", 0) }, { env_u32("HSRLE_MONO_REGION", 0) }, { env_u32("HSRLE_MONO_LOOKBACK", 0) } };

static MonoPlan plan_mono(int codec, uint32_t U, uint32_t C, uint32_t p0, uint32_t spacing = 0u)
{
  MonoPlan m;
  // output bytes per decode lane: enough lanes to fill the GPU (>= 2^18 where the stream allows it), at most the container's 4 KiB
  uint32_t B = pow2_floor((uint64_t)U >> 18);
  B = B < 256u ? 256u : (B > 4096u ? 4096u : B);
  // stream bytes per index lane, and the look-back of its entry guess
  uint32_t G = pow2_floor((uint64_t)C >> 15);
  G = G < 2048u ? 2048u : (G > 8192u ? 8192u : G);
  const uint32_t tB = g_monoTune[0], tG = g_monoTune[1], tM = g_monoTune[2];   // tuning / test knobs (hsrle_mono_tuning, HSRLE_MONO_* in the environment)
  if (tB >= 128u && tB <= (1u << 20) && (tB % 128u) == 0u) B = tB;
  if (spacing != 0u) B = spacing;                                            // (a persistent index: the caller's record spacing, validated by the caller)
  if (tG >= 32u && tG <= (1u << 24)) G = tG;
  m.B = B; m.G = G;
  // Look-back of the entry guess.  Formats with the 7-bit-or-4-byte range field (8 bit Packed, byte-aligned Packed) kill a walk that
  // starts at a wrong byte within a few hops (every other junk range byte claims a 4-byte literal count that points outside the
  // stream), so 1 KiB in front of a region is plenty.  The other formats' junk walks live on and only find the chain by falling onto
  // one of its packet starts (1 hop in ~40 on random literals): they start with 4 KiB, and mono_decode_dev widens the look-back when
  // too many guesses turn out wrong.
  const bool range7 = hsrle::range7(kCodecs[codec]);
  // (range7 formats: regions of at most 4 KiB -- their guesses hold with a 2 KiB look-back, and the walk is one latency chain per region:
  //  the 1 GiB stream 1.47 -> 1.32 ms with 142 191 regions instead of 71 096, none guessed wrong; round 4, since the resolve pass scales)
  if (range7 && G > 4096u && !(tG >= 32u && tG <= (1u << 24))) { G = 4096u; m.G = G; }
  // (range7: 1 KiB leaves ~1 wrong guess in 7 000 on random literals, and each wrong guess costs a repair walk + a second resolve pass:
  //  2 KiB -- none in 71 096 -- where the regions are large enough to carry it: 1 GiB stream 2.28 -> 1.79 ms)
  m.M = tM ? tM : (range7 ? (G >= 4096u ? 2048u : 1024u) : 4096u);
  m.range7 = range7;
  m.R = (uint32_t)(((uint64_t)(C - p0) + G - 1u) / G);
  if (m.R == 0u) m.R = 1u;
  m.KE = (uint32_t)state_slots(kCodecs[codec]);
  m.nb = ((uint64_t)U + B - 1u) / B;
  const uint64_t ks = m.KE ? m.KE : 1u;
  uint64_t at = 0;
  m.offG = at; at += align_up(4ull * m.R, 256);
  m.offE = at; at += align_up(4ull * m.R, 256);
  m.offOlen = at; at += align_up(8ull * m.R, 256);
  m.offT = at; at += align_up(4ull * m.R * ks, 256);
  m.offEntry = at; at += align_up(4ull * m.R, 256);
  m.offOutStart = at; at += align_up(8ull * m.R, 256);
  m.offStateIn = at; at += align_up(4ull * m.R * ks, 256);
  m.offFix = at; at += align_up(4ull * m.R, 256);
  m.offList = at; at += align_up(4ull * m.R, 256);
  m.offMark = at; at += align_up(4ull * m.R, 256);        // (mark | ctrl | rec stay neighbours in this order: mono_prepare clears [offMark, offFast) in one launch)
  m.offCtrl = at; at += 256;
  m.offRec = at; at += align_up(4ull * kEntryRecDwords * m.nb, 256);
  m.offFast = at; at += 256;                                             // the parallel resolve passes: flag + carries, totals per batch of 1 024 regions
  m.offBatch = at; at += align_up(4ull * kFastBatchWords * ((uint64_t)m.R / kResolveThreads + 1ull), 256);
  m.total = at;
  return m;
}

__global__ void k_set_word(uint32_t *p, uint32_t v) { *p = v; }

static hipError_t launch_resolve(const MonoPlan &m, uint8_t *ws, uint32_t p0, uint64_t U, uint32_t roundTag, hipStream_t st)
{
  // the full batches but the last in parallel when every guess is right (hsrle_index.hip.h: k_resolve_fast_*); k_index_resolve finishes -- or, when
  // a region failed the check, does everything
  const uint32_t fastBatches = (m.R > 2u * (uint32_t)kResolveThreads) ? (m.R - 1u) / (uint32_t)kResolveThreads : 0u;
  uint32_t *fast = (uint32_t *)(ws + m.offFast), *batch = (uint32_t *)(ws + m.offBatch);
  const uint32_t *cg = (const uint32_t *)(ws + m.offG), *ce = (const uint32_t *)(ws + m.offE), *ct = (const uint32_t *)(ws + m.offT);
  const uint64_t *col = (const uint64_t *)(ws + m.offOlen);
  if (fastBatches != 0u) hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, st, fast, 1u);      // (a kernel, not a memset node: see mono_prepare)
#define HSRLE_RESOLVE(KE)                                                                                                                                        \
  if (fastBatches != 0u)                                                                                                                                         \
  {                                                                                                                                                              \
    hipLaunchKernelGGL(k_resolve_fast_totals<KE>, dim3(fastBatches), dim3(kResolveThreads), 0, st, cg, ce, col, ct, p0, m.G, fast, batch);                       \
    hipLaunchKernelGGL(k_resolve_fast_carries<KE>, dim3(1), dim3(kResolveThreads), 0, st, fast, batch, fastBatches);                                             \
    hipLaunchKernelGGL(k_resolve_fast_emit<KE>, dim3(fastBatches), dim3(kResolveThreads), 0, st, cg, col, ct, (const uint32_t *)fast, (const uint32_t *)batch,    \
                       (uint32_t *)(ws + m.offEntry), (uint64_t *)(ws + m.offOutStart), (uint32_t *)(ws + m.offStateIn));                                        \
  }                                                                                                                                                              \
  hipLaunchKernelGGL(k_index_resolve<KE>, dim3(1), dim3(kResolveThreads), 0, st, cg, ce, col, ct, m.R, p0, m.G, U, (uint32_t *)(ws + m.offEntry),               \
                     (uint64_t *)(ws + m.offOutStart), (uint32_t *)(ws + m.offStateIn), (uint32_t *)(ws + m.offFix), (uint32_t *)(ws + m.offList),                \
                     (uint32_t *)(ws + m.offCtrl), (uint32_t *)(ws + m.offMark), roundTag, fastBatches ? (const uint32_t *)fast : (const uint32_t *)nullptr, fastBatches)
  switch (m.KE)
  {
  case 0: HSRLE_RESOLVE(0); break;
  case 1: HSRLE_RESOLVE(1); break;
  case 3: HSRLE_RESOLVE(3); break;
  default: HSRLE_RESOLVE(7); break;
  }
#undef HSRLE_RESOLVE
  return hipGetLastError();
}

// what the first bytes of a stream say (reference: rle8_extreme_cpu.h:704-712, :759-760, rleX_extreme_cpu.h:84-91, rleX_Xsl.h:1850-1858)
struct MonoHeader
{
  uint32_t U, C, p0, single, singleSym;
  int codec;   // the id whose kernels decode it (Single mode streams of ids 0 / 1 -> ids 4 / 5)
};

static bool mono_header(int codec, const uint8_t *h16, uint32_t inSize, uint32_t outSize, MonoHeader *mh)
{
  if (codec < 0 || codec >= kCodecCount)
    return false;
  const uint32_t hs = header_size(kCodecs[codec]);
  if (inSize < hs)
    return false;
  memcpy(&mh->U, h16, 4);
  memcpy(&mh->C, h16 + 4, 4);
  if (mh->U > outSize || mh->C > inSize)
    return false;
  if (hs == 9 && h16[8] > 1) // unknown mode (rle8_extreme_cpu.h:759-760)
    return false;
  mh->single = 0; mh->singleSym = 0; mh->p0 = hs; mh->codec = codec;
  if (hs == 9 && h16[8] == 1)
  {
    // rle8_decompress / rle8_packed_decompress switch on the mode byte (rle8_extreme_cpu.h:702-764): Single mode -> the general kernel
    if (codec == HSRLE_RLE8_MULTI) mh->codec = HSRLE_RLE8_SINGLE;
    if (codec == HSRLE_RLE8_PACKED_MULTI) mh->codec = HSRLE_RLE8_PACKED_SINGLE;
    mh->single = 1; mh->singleSym = h16[9]; mh->p0 = 10;
  }
  else if (kCodecs[codec].fam == SHORT_SINGLE) { mh->singleSym = h16[8]; mh->p0 = 9; }   // rleX_Xsl_short.h:1211-1216
  if (mh->U == 0 || mh->C < mh->p0 + 2u || mh->C > 0x7FFFFF00u)
    return false;
  return true;
}

// ---- monolithic decode.  The passes in stream order: walk (every region from a guessed entry) -> resolve (chains the regions, checks the
//      guesses; verdict in ctrl[0..3]) -> records (decoder state at every B output bytes) -> decode.  Since round 5 the records pass is GATED on
//      the verdict on the device and the whole sequence is enqueued without the host in between: a stream whose guesses all hold (the normal
//      case) costs ONE host read at the end instead of two round trips (and none at all through hsrle_decompress_mono_dev_async, which a
//      HIP graph can capture); a stream that needs repair finds zero records, its decode lanes end at once, and the host-driven repair loop
//      takes over where the resolve pass stopped.
__global__ __launch_bounds__(256) void k_mono_clear(u32x4 *__restrict__ p, uint64_t n16)
{
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n16) p[i] = u32x4{ 0, 0, 0, 0 };
}

struct MonoRun
{
  IndexArgs ia;
  uint32_t *ctrl;
  DecodeArgs da;
};

static int mono_prepare(const MonoHeader &mh, const uint8_t *dStream, uint8_t *dOut, uint8_t *ws, const MonoPlan &m, MonoRun *run, hipStream_t st)
{
  init_tables();
  if (!g_launch[mh.codec].dec || !g_launch[mh.codec].idx)
    return HSRLE_ERR_UNSUPPORTED;
  uint32_t *ctrl = (uint32_t *)(ws + m.offCtrl);
  // mark | ctrl | records are neighbours in the workspace (plan_mono), every piece a multiple of 256 bytes: ONE clearing launch.  (Not
  // hipMemsetAsync, whose node misbehaves in a captured and replayed HIP graph -- hsrle_common.hip.h zero_async; seen again here: junk in ctrl[4..15].)
  {
    const uint64_t bytes = m.offFast - m.offMark;
    hipLaunchKernelGGL(k_mono_clear, dim3((uint32_t)((bytes / 16u + 255u) / 256u)), dim3(256), 0, st, (u32x4 *)(ws + m.offMark), bytes / 16u);
    if (hipGetLastError() != hipSuccess)
      return HSRLE_ERR_DEVICE;
  }

  IndexArgs ia{};
  ia.stream = dStream; ia.C = mh.C; ia.p0 = mh.p0; ia.G = m.G; ia.M = m.M; ia.R = m.R; ia.single = mh.single; ia.singleSym = mh.singleSym;
  ia.list = nullptr; ia.listCount = 0; ia.fix = (const uint32_t *)(ws + m.offFix);
  ia.g = (uint32_t *)(ws + m.offG); ia.e = (uint32_t *)(ws + m.offE); ia.olen = (uint64_t *)(ws + m.offOlen); ia.t = (uint32_t *)(ws + m.offT);
  ia.entry = (const uint32_t *)(ws + m.offEntry); ia.outStart = (const uint64_t *)(ws + m.offOutStart); ia.stateIn = (const uint32_t *)(ws + m.offStateIn);
  ia.U = mh.U; ia.B = m.B; ia.rec = (uint32_t *)(ws + m.offRec);
  ia.mark = (uint32_t *)(ws + m.offMark); ia.roundTag = 0;
  { static const uint32_t ext = env_u32("HSRLE_MONO_REPAIR_EXTEND", 48); ia.extMax = ext; }
  run->ia = ia;
  run->ctrl = ctrl;
  run->da = DecodeArgs{ dStream, nullptr, dStream + mh.C + HSRLE_CONTAINER_TAIL_PAD, dOut, mh.U, m.B, 0u, (uint32_t)m.nb, ctrl + 8 };
  run->da.entries = (const uint32_t *)(ws + m.offRec);
  run->da.entryBase = 0;
  return HSRLE_OK;
}

// walk of every region, resolve round 1, gated records, decode (unless only the index is wanted): nothing here waits for the host
static int mono_enqueue_first_try(const MonoHeader &mh, uint8_t *ws, const MonoPlan &m, MonoRun &run, hipStream_t st, bool decode = true)
{
  if (g_launch[mh.codec].idx(run.ia, 0, st) != hipSuccess || launch_resolve(m, ws, mh.p0, mh.U, 1u, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  run.ia.gate = run.ctrl;
  const hipError_t e = g_launch[mh.codec].idx(run.ia, 1, st);
  run.ia.gate = nullptr;
  run.da.gate = run.ctrl;                                                // (the decode too: nothing to decode from records that were not written)
  const hipError_t e2 = (e != hipSuccess || !decode) ? e : g_launch[mh.codec].dec(run.da, st);
  run.da.gate = nullptr;
  if (e2 != hipSuccess)
    return HSRLE_ERR_DEVICE;
  return HSRLE_OK;
}

// ctrl[0] regions whose guess failed, ctrl[1] malformed stream, ctrl[8] the decode kernel's error bits -> one word for the caller
__global__ void k_mono_status(const uint32_t *__restrict__ ctrl, uint32_t *__restrict__ status)
{
  *status = ctrl[1] != 0u ? (uint32_t)HSRLE_MONO_MALFORMED : (ctrl[0] != 0u ? (uint32_t)HSRLE_MONO_NEEDS_REPAIR : (ctrl[8] != 0u ? (uint32_t)HSRLE_MONO_MALFORMED : (uint32_t)HSRLE_MONO_DONE));
}

// dStream: 128-byte aligned, readable up to C + 64.  stats (optional): [0] regions, [1] repair rounds, [2] regions walked again.
// Synchronises the stream (once when every guess holds; the repair loop reads the resolve pass's verdict per round).
// recOut != nullptr: the persistent index (hsrle_mono_index_build_dev) -- the proven records go to recOut (m.nb records, cleared here first)
// instead of the workspace, and nothing is decoded (dOut is not used).
// Returns HSRLE_OK / HSRLE_ERR_FORMAT / HSRLE_ERR_DEVICE.
static int mono_decode_dev(const MonoHeader &mh, const uint8_t *dStream, uint8_t *dOut, uint8_t *ws, const MonoPlan &m, uint32_t *stats, hipStream_t st,
                           uint32_t *recOut = nullptr)
{
  MonoRun run;
  const int prc = mono_prepare(mh, dStream, dOut, ws, m, &run, st);
  if (prc != HSRLE_OK)
    return prc;
  IndexArgs &ia = run.ia;
  uint32_t *const ctrl = run.ctrl;
  const bool decode = recOut == nullptr;
  if (!decode)
  {
    // (every dword of every record is written -- the ones a codec's state does not use as zeros -- so the index bytes depend on the stream alone)
    ia.rec = recOut;
    const uint64_t n16 = m.nb * kEntryRecDwords / 4u;
    hipLaunchKernelGGL(k_mono_clear, dim3((uint32_t)((n16 + 255u) / 256u)), dim3(256), 0, st, (u32x4 *)recOut, n16);
    if (hipGetLastError() != hipSuccess)
      return HSRLE_ERR_DEVICE;
  }
  if (!m.range7 && m.R >= 16384u && g_monoTune[2] == 0u)                  // (small streams: the pilot's launch + read costs more than a widened second try)
  {
    // formats whose junk walks do not die: does the short look-back find the chain on THIS stream?  A pilot over the first 128 regions
    // tells (data with little entropy synchronises within bytes, random literals need ~16 KiB): each wrong guess costs a repair later
    uint32_t pg[128], pe[128];
    IndexArgs pilot = ia;
    pilot.R = 128u;
    if (g_launch[mh.codec].idx(pilot, 0, st) != hipSuccess || hipMemcpyAsync(pg, ia.g, sizeof(pg), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(pe, ia.e, sizeof(pe), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
    uint32_t agree = 0;
    for (uint32_t r = 1; r < 128u; r++) agree += (pe[r - 1] == pg[r]) ? 1u : 0u;
    if (agree < 120u) ia.M = 16384u;
  }
  uint32_t rounds = 0, rewalked = 0, roundTag = 1;
  uint32_t verdict[12] = { 0 };                                            // [0..3] the resolve pass's verdict, [8] the decode kernel's status
  if (mono_enqueue_first_try(mh, ws, m, run, st, decode) != HSRLE_OK ||
      hipMemcpyAsync(verdict, ctrl, 36, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  if (verdict[0] == 0u)
  {
    if (stats) { stats[0] = m.R; stats[1] = 0; stats[2] = 0; stats[3] = ia.M; }
    return (verdict[1] != 0u || verdict[8] != 0u) ? HSRLE_ERR_FORMAT : HSRLE_OK;
  }
  for (;;)
  {
    if (rounds++ > m.R)                                    // every round proves at least one more region: cannot happen
      return HSRLE_ERR_DEVICE;
    rewalked += verdict[0];
    if (rounds == 1u && verdict[0] > 8u && verdict[0] > m.R / 32u && ia.M < 65536u && g_monoTune[2] == 0u)
    {
      // the guesses of this stream do not find the chain within the look-back (wrong guesses come in streaks, and a streak is repaired
      // one region per round): guess again, everywhere, from four times as far back
      ia.M *= 4u;
      ia.list = nullptr; ia.listCount = 0;
      rounds = 0;
    }
    else { ia.list = (const uint32_t *)(ws + m.offList); ia.listCount = verdict[0]; ia.roundTag = roundTag; }
    if (g_launch[mh.codec].idx(ia, 0, st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
    roundTag++;
    if (launch_resolve(m, ws, mh.p0, mh.U, roundTag, st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
    if (hipMemcpyAsync(verdict, ctrl, 16, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
    if (verdict[0] == 0u)
      break;
  }
  if (stats) { stats[0] = m.R; stats[1] = rounds; stats[2] = rewalked; stats[3] = ia.M; }
  if (verdict[1] != 0u)
    return HSRLE_ERR_FORMAT;

  // (the first try's decode lanes found zero records and left their error bits in the status word)
  ia.list = nullptr; ia.listCount = 0;
  if (!decode)
    return g_launch[mh.codec].idx(ia, 1, st) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
  hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, st, ctrl + 8, 0u);
  if (g_launch[mh.codec].idx(ia, 1, st) != hipSuccess || g_launch[mh.codec].dec(run.da, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  uint32_t status = 1;
  if (hipMemcpyAsync(&status, ctrl + 8, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  return status == 0u ? HSRLE_OK : HSRLE_ERR_FORMAT;
}

} // namespace hsrle
