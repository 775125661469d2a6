// hsrle_capi_container.h -- part of hsrle_capi.hip: workspace plan, the encode rule's host side and the encode paths, the cut finders' launcher, the decode prologue, block / split / wave decode
#pragma once
#include "hsrle_capi_kernels.h"
#include "hsrle_expand.hip.h"
#include "hsrle_mono_encode.hip.h"
#ifdef HSRLE_EXPERIMENTS
#include "experiments/hsrle_encode8w.hip.h"
#else
namespace hsrle { constexpr uint64_t kTicketBytes = 256; }   // (scratch behind the staging slots: the ring choice of the 1 / 2 byte encoders lives there)
#endif

namespace hsrle {

// workspace layout: [slots][sizes u32][level-1 sums u64][level-2 sums u64][level-3 sums u64]
// Optionally (EncodeKnobs::chunkBlocks) inputs are compressed CHUNK by chunk: the compaction of chunk k (bandwidth bound, no LDS) runs on a
// second stream while the encode kernel (latency bound, LDS limited to 9 waves per CU) works on chunk k + 1, and the staging slots are
// two chunks' worth instead of the whole input's (8 GiB: 2.3 GB instead of 9 GB).  The scan of a chunk's stream sizes starts at the
// running total the previous chunk left in the offset table.  OFF by default: measured on the 8 GiB headline buffer the overlap does not pay -- 1 130 GiB/s in one piece against 846 / 964 / 1 015 /
// 1 063 GiB/s with chunks of 131 072 / 262 144 / 524 288 / 1 048 576 blocks (the compaction's traffic slows the encode kernel by more
// than its own 1.8 ms, and every chunk boundary drains the GPU).  HSRLE_ENCODE_CHUNK_BLOCKS=n turns it on for callers that would rather
// have the smaller workspace (two chunks of staging slots instead of the whole input's).
// Windowed encoders: containers of blocks above 4 KiB whatever their size -- 8 MiB of 8 KiB / 64 KiB blocks 19 / 51 us against 211 / 1 187 us of the split encode, 8 GiB 5.0 / 5.0 ms
// against 7.4 / 7.6 of the ring encoders + k_compact (1 MiB blocks: 5.5 against 20.7; experiments/r06, calls 22, 25)
#ifndef HSRLE_PPW_MIN_BLOCKS
#define HSRLE_PPW_MIN_BLOCKS 1u
#endif
constexpr uint32_t kPpwMinBlocks = HSRLE_PPW_MIN_BLOCKS;   // (A/B builds: 0xFFFFFFFF = never, also for the monolithic streams)
static_assert(kEncodeWaveBytes == kPpMaxBlock && kEncodeWaveBytes == kPpwWindow, "the rule's block / window size is the kernels'");
// the knobs of the encode rule (hsrle_codecs.h: encode_choice), read once; the shipped build has the defaults
static const EncodeKnobs &encode_knobs()
{
#ifdef HSRLE_EXPERIMENTS
  static const EncodeKnobs k{ knob_u32("HSRLE_PP", 0u), knob_u32("HSRLE_RUNLIST", 0u), knob_u32("HSRLE_ENCODE_WAVE", 0u) != 0u ? kWaveEncodeMaxBlock : 0u, kPpwMinBlocks,
                              knob_u32("HSRLE_ENCODE_CHUNK_BLOCKS", 0u), SPLIT_ALL };
#else
  static const EncodeKnobs k{ 0u, 0u, 0u, kPpwMinBlocks };
#endif
  return k;
}
// the rule for a codec id: what the row has comes from the launch table
static EncodeChoice encode_choice_of(int codec, uint64_t U, uint32_t B, SplitRegions have, bool noSplit = false)
{
  init_tables();
  const CodecLaunch &l = g_launch[codec];
  const EncodeCaps caps{ l.pp != nullptr, l.ppw8 ? PPW_8 : (l.ppwL ? PPW_L : (l.ppwS ? PPW_S : PPW_NONE)), l.menc != nullptr, l.enc != nullptr, l.wenc != nullptr };
  return encode_choice(kCodecs[codec], caps, U, B, block_count(U, B), have, noSplit, encode_knobs());
}

// Split encode (hsrle_mono_encode.hip.h): containers with too few blocks for one lane each are encoded chunk by chunk -- the blocks cut behind
// runs every encoder state stores, like a monolithic stream, with the block starts as forced cuts.  kSplitPieces pieces (= cut finder lanes) per block.
struct Workspace
{
  uint64_t nBlocks, chunk, nChunks;
  // split encode: cut finder results per piece, chunk table, sizes / offsets per chunk, lists (8 words per chunk), staging slots
  uint64_t spCutPos, spCutSym, spFlags, spIdx, spStarts, spSyms, spSlotOff, spSizes, spChunkOff, spFirst, spCtrl, spGuess, spListOut, spSlots, spPieces, spMaxChunks, spPick, spJobs, spJobCap;
  ScanLevels levels, spLevels;   // of the size scan over the blocks / of the split encode's scans (flags per piece, sizes per chunk)
  uint64_t offSlots, offSizes, total;
};

// regions: which split-encode regions to reserve (EncodeChoice::regions; without a codec: what every caller's workspace has)
static Workspace plan_workspace(uint64_t U, uint32_t B, SplitRegions regions = encode_knobs().generic)
{
  Workspace w{};                                                          // (regions that are not reserved stay 0)
  w.nBlocks = block_count(U, B);
  w.chunk = encode_chunk(w.nBlocks, encode_knobs());
  w.nChunks = (w.nBlocks + w.chunk - 1) / w.chunk;
  const uint64_t slotBlocks = w.nChunks > 1 ? 2u * w.chunk : w.nBlocks;
  uint64_t at = 0;
  w.offSlots = at; at += align_up(slotBlocks * (uint64_t)slot_stride(B) + kTicketBytes, 256);    // (+ the wave encoder's counters: hsrle_encode8w.hip.h)
  w.offSizes = at; at += align_up(w.nBlocks * 4ull, 256);
  w.levels.lay_out(w.chunk, at);
  // (split encode regions: sized for every codec, but only where the split path can run -- small containers of blocks above 4 KiB; up to
  //  4 KiB the run list encoders take every codec that has a chunk mode, and reserving the regions there cost 3x the input for nothing:
  //  ADVICE r3 -- SPLIT_ALL is for the codecs that have none.  SPLIT_NONE: a codec whose blocks above 4 KiB go to the windowed encoders.)
  w.spPieces = w.nBlocks * kSplitPiecesMax; w.spMaxChunks = w.spPieces + w.nBlocks;
  if (w.nBlocks < kSplitEncodeBelow && B >= 1024u && B <= (1u << 20) && (regions == SPLIT_ALL || (regions == SPLIT_LARGE && B > kEncodeWaveBytes)))
  {
    const uint64_t np = w.spPieces, nc = w.spMaxChunks;
    w.spCutPos = at; at += align_up(8ull * np, 256);
    w.spCutSym = at; at += align_up(8ull * np, 256);
    w.spFlags = at; at += align_up(4ull * np, 256);
    w.spIdx = at; at += align_up(8ull * (np + 1), 256);
    w.spStarts = at; at += align_up(8ull * (nc + 2), 256);
    w.spSyms = at; at += align_up(8ull * (nc + 1), 256);
    w.spSlotOff = at; at += align_up(8ull * (nc + 1), 256);
    w.spSizes = at; at += align_up(4ull * (nc + 1), 256);
    w.spChunkOff = at; at += align_up(8ull * (nc + 2), 256);
    w.spCtrl = at; at += 256;                                            // (the table of first chunks follows the control words directly: the ring encoders find it at ctrl + 64)
    w.spFirst = at; at += align_up(4ull * (w.nBlocks + 2), 256);
    w.spGuess = at; at += align_up(64ull * (nc + 1), 256);
    w.spListOut = at; at += align_up(64ull * (nc + 1), 256);
    w.spLevels.lay_out(nc + 2, at);
    w.spPick = at; at += align_up(w.nBlocks + 16ull, 256);               // 8 bit Single: a symbol per block
    w.spJobCap = (U >> 10) + nc + 16ull;                                  // ... and its copy jobs (literal stretches of >= 1 KiB go to whole waves: k_copy_jobs)
    w.spJobs = at; at += align_up(24ull * w.spJobCap, 256);
    w.spSlots = at; at += align_up(U + (U >> 7) + 256ull * (nc + 2) + 4096ull, 256);
  }
  w.total = at;
  return w;
}

// the device's second stream (compaction behind the encode kernel); created once, shared by concurrent calls (their compactions then
// simply queue up behind each other)
static hipStream_t aux_stream()
{
  DeviceState &D = this_device();
  std::lock_guard<std::mutex> lock(D.mu);
  if (!D.aux && hipStreamCreateWithFlags(&D.aux, hipStreamNonBlocking) != hipSuccess) D.aux = nullptr;
  return D.aux;
}

// ------------------------------------------------------------------------------------------------------------------
// split encode of a container: the cut finders (also those of the monolithic encode, hsrle_capi_mono_encode.h), its predicates, compress_split

// the cut finders (hsrle_mono_encode.hip.h) by symbol width and alignment, one lane per piece of G bytes; the run length that makes a cut: hsrle_codecs.h cut_long().
// onlySym (8 bit symbols; device): the Single codecs' symbol -- only its runs are cuts.  blockB != 0: the pieces are those of a container's blocks.
static void launch_cuts(int S, int aligned, const uint32_t *onlySym, dim3 grid, hipStream_t st, const uint8_t *dIn, uint64_t U, uint32_t G, uint32_t pieces, uint32_t longc,
                        uint64_t *cutPos, uint64_t *cutSym, uint32_t *flags, uint32_t blockB = 0)
{
#define HSRLE_CUTS(SS) \
  if (aligned) hipLaunchKernelGGL((k_mono_cutsS<SS, 1>), grid, dim3(64), 0, st, dIn, U, G, pieces, longc, cutPos, cutSym, flags, blockB); \
  else hipLaunchKernelGGL((k_mono_cutsS<SS, 0>), grid, dim3(64), 0, st, dIn, U, G, pieces, longc, cutPos, cutSym, flags, blockB)
  switch (S)
  {
  case 1: hipLaunchKernelGGL(k_mono_cuts8, grid, dim3(64), 0, st, dIn, U, G, pieces, longc, cutPos, cutSym, flags, onlySym, blockB); break;
  case 16: HSRLE_CUTS(16); break;
  case 2: HSRLE_CUTS(2); break;
  case 3: HSRLE_CUTS(3); break;
  case 4: HSRLE_CUTS(4); break;
  case 6: HSRLE_CUTS(6); break;
  default: HSRLE_CUTS(8); break;
  }
#undef HSRLE_CUTS
}

// pieces per block (= cut finder lanes; a block has at most pieces + 1 chunks).  8 pieces were measured for the list codecs that settle their
// lists inside the encode kernel (88 MB frame / 64 MiB runs, us: rle64_3symlut_byte 4: 310 / 378, 8: 341 / 485; rle32_7symlut_sym 4: 411 / 355,
// 8: 409 / 328; rle16_3symlut_byte 4: 434 / 315, 8: 497 / 327): the kernel's time follows its total trips, not the trips per wave, so
// shorter chunks buy nothing; the per-lane chunk encoders (Single, 128 bit, Greedy with a one-symbol list), 4 / 8 pieces: rle8_single 285 / 290 and 379 / 365,
// rle128_sym 380 / 374 and 282 / 324, rle64_1symlut greedy 732 / 689 and 775 / 1029 (experiments/r04/call61.sh).  The workspace is planned for kSplitPiecesMax so that experiment builds can try (HSRLE_SPLIT_PIECES).
static uint32_t split_pieces(uint32_t B)
{
  const uint32_t k = knob_u32("HSRLE_SPLIT_PIECES", kSplitPieces);
  return (k == kSplitPiecesMax && B % (kSplitPiecesMax * 128u) == 0u) ? k : kSplitPieces;
}

// Split encode of a container (no host synchronisation: graph capturable like the plain path): cuts inside the blocks -> chunk table (block
// starts are forced cuts) -> the ring encoders' chunk mode with B given (headers at block starts, the block's end as the end of the input) ->
// for the list codecs: every chunk from the default list, then the proof and kSplitPieces repair rounds (a chunk's list is wrong only if
// a chunk in front of it IN ITS BLOCK stored a symbol the default list does not lead with; a round makes one more chunk per block right) ->
// size scan over the chunks, placement, offset table + compressedLength fields.
static int compress_split(int codec, const uint8_t *dIn, uint64_t U, uint32_t B, uint32_t nBlocks, uint8_t *ws, const Workspace &w, uint64_t *offsets, uint8_t *payload, hipStream_t st)
{
  const CodecInfo &ci = kCodecs[codec];
  const int S = ci.S, listK = list_len(ci);
  const uint32_t longc = cut_long(ci);
  const uint32_t ppb = split_pieces(B);
  const uint32_t G = B / ppb, pieces = nBlocks * ppb, maxChunks = pieces + nBlocks;
  uint64_t *cutPos = (uint64_t *)(ws + w.spCutPos), *cutSym = (uint64_t *)(ws + w.spCutSym), *idx = (uint64_t *)(ws + w.spIdx), *starts = (uint64_t *)(ws + w.spStarts);
  uint64_t *syms = (uint64_t *)(ws + w.spSyms), *slotOff = (uint64_t *)(ws + w.spSlotOff), *chunkOff = (uint64_t *)(ws + w.spChunkOff);
  uint64_t *guess = (uint64_t *)(ws + w.spGuess), *listOut = (uint64_t *)(ws + w.spListOut);
  uint32_t *flags = (uint32_t *)(ws + w.spFlags), *sizes = (uint32_t *)(ws + w.spSizes), *firstChunk = (uint32_t *)(ws + w.spFirst), *ctrl = (uint32_t *)(ws + w.spCtrl);
  const ScanLevels &sw = w.spLevels;
  static_assert(9u + kSplitPiecesMax - 1u <= 16u, "the list-verify rounds count into ctrl[9 + round]: below the verdict flag ctrl[24]");
  if (zero2_async(ctrl, 128, sizes, 4ull * (maxChunks + 1ull), st) != hipSuccess)   // (graph capturable: not hipMemsetAsync, see zero_async; 256 bytes are reserved)
    return HSRLE_ERR_DEVICE;
  const dim3 cgrid((pieces + 63u) / 64u);
  const bool single = is_single(ci);
  uint32_t *const pickTable = (uint32_t *)(ws + w.spPick);             // (8 bit Single: a byte per block)
  if (single)
  {
    // every block's symbol first (k_single_pick through the codec's launcher): only its runs are cuts, and the chunk encoder needs it
    EncodeArgs pa{ dIn, U, B, nBlocks, nullptr, 0u, nullptr };
    MonoEncodeArgs pm{ nullptr, nullptr, nullptr, 0u };
    pm.pick = pickTable; pm.phase = 1u;
    pm.cutPos = cutPos; pm.cutSym = cutSym; pm.cutFlags = flags; pm.cutG = G; pm.cutLong = longc;   // (... and the blocks' cuts, by the same waves: the block is in LDS there)
    if (g_launch[codec].menc(pa, pm, st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
  }
  if (!single) launch_cuts(S, ci.aligned, nullptr, cgrid, st, dIn, U, G, pieces, longc, cutPos, cutSym, flags, B);   // (Single: the pick above left the cuts)
  if (scan_sizes(flags, pieces, idx, ws, sw, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  if (listK != 0)
    hipLaunchKernelGGL(k_mono_list_default, dim3((maxChunks + 255u) / 256u), dim3(256), 0, st, maxChunks, (uint32_t)listK, (uint32_t)S, guess);
  // list codecs of 2 .. 8 byte symbols settle their lists INSIDE the encode kernel: a wave takes the chunks of kSplitGroup whole blocks (k_encodeS_blocks)
  const uint32_t kSplitGroup = 64u / (ppb + 1u);                         // blocks per wave: x (ppb + 1) chunks at most <= a wave's 64 lanes
  const bool inKernelLists = listK != 0 && S > 1 && !ci.greedy;   // (Greedy: one lane per chunk, lists between launches like the 8 bit codecs)
  hipLaunchKernelGGL(k_split_scatter, dim3((pieces + 255u) / 256u), dim3(256), 0, st, (const uint64_t *)cutPos, (const uint64_t *)cutSym, (const uint32_t *)flags, (const uint64_t *)idx, pieces,
                     ppb, nBlocks, U, B, starts, listK ? guess : syms, slotOff, firstChunk, ctrl, (uint32_t)listK | (greedy_one_symbol_list(ci) ? kSplitGuessCutSym : 0u), inKernelLists ? kSplitGroup : 0u);

  EncodeArgs ea{ dIn, U, B, inKernelLists ? ((nBlocks + kSplitGroup - 1u) / kSplitGroup) * 64u : maxChunks, ws + w.spSlots, 0u, sizes };
  ea.ringSel = ctrl;                                                     // chunk mode with B: ctrl[0] = the number of chunks, [1] = blocks per wave (0: chunks in a row), [2] = blocks
  MonoEncodeArgs ma{ starts, listK ? guess : syms, slotOff, 2u * (B / 64u) + 64u };
  ma.listOut = listK ? listOut : nullptr;
  ma.pick = pickTable;                                                 // (8 bit Single: the blocks' symbols)
  if (single) { ma.jobs = (uint64_t *)(ws + w.spJobs); ma.jobCount = ctrl + 12; ma.jobCap = (uint32_t)(w.spJobCap < 0xFFFFFFFFull ? w.spJobCap : 0xFFFFFFFFull); }   // (ctrl[12]: zeroed above)
  if (g_launch[codec].menc(ea, ma, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  if (listK != 0 && !inKernelLists)
  {
    // (8 bit symbols: between launches.)  What every chunk does to a list is known from the first pass: the lists in front of all chunks at once, then the chunks whose list is
    // not the default one again (run-distributed rle64_3symlut_byte: every chunk).  Then the proof, with repair: a re-encoded chunk may store
    // other runs than it did from the default list and leave another list behind; after the pass above the first two chunks of every block are
    // final, every verify round makes one more so, and a block has at most kSplitPieces + 1 chunks.  The rounds tell the encoder which
    // counter says whether they have anything to do (an empty round is two launches that return at once).
    const uint32_t base = ma.steps;
    hipLaunchKernelGGL(k_split_list_guess, dim3((maxChunks + 255u) / 256u), dim3(256), 0, st, guess, (const uint64_t *)listOut, (const uint64_t *)starts, (const uint32_t *)ctrl, B, (uint32_t)listK, (uint32_t)S,
                       ctrl + 8);
    ma.steps = base | (1u << 16);
    if (g_launch[codec].menc(ea, ma, st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
    for (uint32_t round = 0; round + 1u < ppb; round++)
    {
      hipLaunchKernelGGL(k_split_list_verify, dim3((maxChunks + 255u) / 256u), dim3(256), 0, st, guess, (const uint64_t *)listOut, (const uint64_t *)starts, (const uint32_t *)ctrl, B, (uint32_t)listK,
                         (uint32_t)S, ctrl + 9 + round);
      ma.steps = base | ((2u + round) << 16);
      if (g_launch[codec].menc(ea, ma, st) != hipSuccess)                       // (chunks whose list was right are switched off: word 7 of their guess)
        return HSRLE_ERR_DEVICE;
    }
  }
  const bool laneChunks = single || S == 16 || ci.greedy;           // per-lane chunk encoders: a chunk that missed its boundary run says so with size 0
  if (laneChunks)
    hipLaunchKernelGGL(k_split_check, dim3((nBlocks + 255u) / 256u), dim3(256), 0, st, (const uint32_t *)firstChunk, (const uint64_t *)starts, (const uint32_t *)sizes, nBlocks, ctrl + 24);   // (ctrl[24]: zeroed above; outside the rounds' counters ctrl[9 ..] and the Single encoders' ctrl[12] -- ADVICE r5)
  if (scan_sizes(sizes, maxChunks, chunkOff, ws, sw, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  launch_compact_var(G <= 2048u, (const uint8_t *)(ws + w.spSlots), (const uint64_t *)slotOff, (const uint64_t *)chunkOff, payload, maxChunks, st);
  // (... and the container's header and tail pad: the caller does not launch k_finish_container behind a split encode)
  uint8_t *const container = (uint8_t *)offsets - HSRLE_CONTAINER_HEADER_SIZE;
  const uint32_t codecId = (uint32_t)codec;
  auto finish = [=] __device__(uint64_t payloadSize) { finish_container(container, codecId, U, B, nBlocks, payloadSize); };
  hipLaunchKernelGGL((k_split_finish<decltype(finish)>), dim3((nBlocks + 255u) / 256u), dim3(256), 0, st, (const uint32_t *)firstChunk, (const uint64_t *)chunkOff, nBlocks, offsets, payload, finish);
  if (laneChunks)
    hipLaunchKernelGGL(k_split_verdict, dim3(1), dim3(64), 0, st, (const uint32_t *)(ctrl + 24), container);
  return hipGetLastError() == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

// The windowed launcher of a codec and the words of its windows' state records: the 8 bit pair 8, the codecs of hsrle_encodeSp.hip.h 16, those of hsrle_encodeLp.hip.h (the
// list travels with it) 32.  Blocks of a container: ppw8, then ppwL, then ppwS.  Chunks of ONE monolithic stream, for the codecs whose encoder state at a cut is fixed by
// the cut itself (hsrle_codecs.h: chunk_mode): ppw8, then ppwSM, the chunk mode of hsrle_encodeSpw.hip.h.  Callers run behind init_tables().
struct PpwPick { PpwLaunch launch; uint32_t stateWords; };
static PpwPick ppw_pick(int codec, bool chunks)
{
  const CodecLaunch &l = g_launch[codec];
  if (chunks) return { !chunk_mode(kCodecs[codec]) ? nullptr : (l.ppw8 ? l.ppw8 : l.ppwSM), l.ppw8 ? kPpwStateWords : kPpwSStateWords };
  return l.ppw8 ? PpwPick{ l.ppw8, kPpwStateWords } : (l.ppwL ? PpwPick{ l.ppwL, kPpwLStateWords } : PpwPick{ l.ppwS, kPpwSStateWords });
}
// states, then (256-byte aligned) the records of nWindows windows from `base` on: the slot area, which the windowed encoders do not stage in
static void ppw_lay_out(PpwArgs &pa, uint8_t *base, uint32_t stateWords, uint64_t nWindows)
{
  pa.nWindows = (uint32_t)nWindows; pa.states = (uint32_t *)base; pa.recs = (uint32_t *)(base + align_up(4ull * stateWords * nWindows, 256));
}

static int compress_async(int codec, const void *dIn, uint64_t U, void *dOut, uint64_t cap, uint32_t B, void *dWs, uint64_t wsSize, hipStream_t st, bool noSplit = false)
{
  if (codec < 0 || codec >= kCodecCount || dIn == nullptr || dOut == nullptr || U == 0)
    return HSRLE_ERR_ARGUMENT;
  if (B == 0) B = HSRLE_DEFAULT_BLOCK_SIZE;
  if (!valid_block_size(B))
    return HSRLE_ERR_ARGUMENT;
  if (cap < hsrle_container_bound(U, B))
    return HSRLE_ERR_CAPACITY;
  if (block_count(U, B) > 0xFFFFFFF0ull)
    return HSRLE_ERR_ARGUMENT;
  if (!device_ok())
    return HSRLE_ERR_DEVICE;

  // (small containers of 1 .. 4 KiB blocks of the codecs without a run list encoder: the split encode needs regions the general workspace does not reserve -- the
  //  library's own scratch has them, a caller's workspace if it was sized by hsrle_compress_workspace_size_codec.  The plan reserves them only where the split
  //  encode will really run: they are 2 - 3 x the input -- ADVICE r4)
  const SplitRegions have = (dWs == nullptr || wsSize >= plan_workspace(U, B, SPLIT_ALL).total) ? SPLIT_ALL : encode_knobs().generic;
  const EncodeChoice ec = encode_choice_of(codec, U, B, have, noSplit);
  if (ec.path == ENC_UNSUPPORTED)
    return HSRLE_ERR_UNSUPPORTED;
  const Workspace w = plan_workspace(U, B, ec.regions);

  void *own = nullptr;
  if (dWs == nullptr)
  {
    own = scratch_alloc(w.total, st);                    // freed (stream-ordered) behind the last kernel below
    if (!own)
      return HSRLE_ERR_DEVICE;
    dWs = own;
  }
  else if (wsSize < w.total)
    return HSRLE_ERR_CAPACITY;

  uint8_t *ws = (uint8_t *)dWs;
  uint8_t *container = (uint8_t *)dOut;
  const uint32_t nBlocks = (uint32_t)w.nBlocks;
  uint64_t *offsets = (uint64_t *)(container + HSRLE_CONTAINER_HEADER_SIZE);
  uint8_t *payload = container + HSRLE_CONTAINER_HEADER_SIZE + 8ull * ((uint64_t)nBlocks + 1ull);
  const uint32_t stride = slot_stride(B);
  uint32_t *sizes = (uint32_t *)(ws + w.offSizes);
  int rc = HSRLE_OK;
  bool finished = false;                                                // (small containers: the size scan's launch wrote header and tail pad)

  // sizes -> offsets.  Small containers: in ONE launch that writes header and tail pad too -- it reads the sizes 16 bytes at a time, and a caller's workspace may sit anywhere
  auto scan_and_place = [&]() -> bool {
    if (nBlocks > kScanSmallMax || (((uintptr_t)sizes) & 15u) != 0u)
      return scan_sizes(sizes, nBlocks, offsets, ws, w.levels, st) == hipSuccess;
    hipLaunchKernelGGL(k_scan_small_finish, dim3((nBlocks + kScanTile - 1u) / kScanTile), dim3(kScanThreads), 0, st, (const uint32_t *)sizes, nBlocks, offsets, container, (uint32_t)codec, U, B);
    finished = true;
    return true;
  };
  switch (ec.path)
  {
#ifdef HSRLE_EXPERIMENTS
  case ENC_WAVE:
  {
    // HSRLE_ENCODE_WAVE=1: rle8_multi / rle8_packed_multi with blocks of at most 4 KiB by ONE WAVE PER BLOCK (hsrle_encode8w.hip.h: position
    // parallel run detection, offsets by decoupled look-back, the payload written once, no staging slots and no compaction pass).  Bit-exact
    // (every block of the 8 GiB buffer against the reference manifest), but OFF by default: at 4 KiB per wave the kernel is bound by the
    // latency chain of one block, not by traffic -- 8 GiB: 13.5 ms against 7.4 ms of the lane-per-block kernel + compaction (input load + masks
    // 2.1 ms, run list 0.7, decisions 2.1, packets 2.6, look-back 1.4 .. 5.9 ms).
    // (the slot area of the lane-per-block path is not needed: the tile words and the ticket counters live at its start)
    uint32_t *ticket = (uint32_t *)(ws + w.offSlots);
    unsigned long long *tiles = (unsigned long long *)(ws + w.offSlots + kTicketBytes);
    WaveEncodeArgs wa{ (const uint8_t *)dIn, U, B, nBlocks, offsets, payload, tiles, ticket };
    if (w.offSizes - w.offSlots < kTicketBytes + 8ull * nBlocks) rc = HSRLE_ERR_CAPACITY;
    else if (zero_async(ticket, kTicketBytes + 8ull * nBlocks, st) != hipSuccess || g_launch[codec].wenc(wa, st) != hipSuccess)
      rc = HSRLE_ERR_DEVICE;
    break;
  }
#endif
  case ENC_PP:
  {
    // position-parallel encoder (hsrle_encode8p.hip.h): sizes + one record per stored run, scan, then every stream written once to its final place --
    // no staging slots, no compaction.  The records live in the (otherwise unused) slot area: pp_scratch_bytes() is less than nBlocks staging slots for every block size.
    PpArgs pa{ (const uint8_t *)dIn, U, B, nBlocks, sizes, offsets, payload, ws + w.offSlots };
    if (g_launch[codec].pp(pa, 0, st) != hipSuccess || !scan_and_place() || g_launch[codec].pp(pa, 1, st) != hipSuccess)
      rc = HSRLE_ERR_DEVICE;
    break;
  }
  case ENC_PPW:
  {
    // the same encoder, a block walked in windows of 4 KiB: a wave per block leaves sizes, window states and records; after the scan a wave per window writes
    // the packets of the runs that end in it.  States and records live in the slot area (1 056 bytes per window).
    const PpwPick pick = ppw_pick(codec, false);
    PpwArgs pa{};
    pa.in = (const uint8_t *)dIn; pa.U = U; pa.B = B; pa.nUnits = nBlocks; pa.sizes = sizes; pa.offsets = offsets; pa.payload = payload;
    ppw_lay_out(pa, ws + w.offSlots, pick.stateWords, (uint64_t)nBlocks * ((B + kPpwWindow - 1u) / kPpwWindow));
    if (pick.launch(pa, 0, st) != hipSuccess || !scan_and_place() || pick.launch(pa, 1, st) != hipSuccess)
      rc = HSRLE_ERR_DEVICE;
    break;
  }
  case ENC_SPLIT:
    rc = compress_split(codec, (const uint8_t *)dIn, U, B, nBlocks, ws, w, offsets, payload, st);
    finished = true;                                                    // (k_split_finish wrote header and tail pad)
    break;
  case ENC_RING:
  {
    EncodeArgs ea{ (const uint8_t *)dIn, U, B, nBlocks, ws + w.offSlots, stride, sizes };
    ea.ringSel = (uint32_t *)(ws + w.offSlots + align_up((uint64_t)nBlocks * stride, 256));   // (in the wave encoder's counter area behind the slots: unused on this path)
    if (g_launch[codec].enc(ea, st) != hipSuccess || !scan_and_place())
      rc = HSRLE_ERR_DEVICE;
    else
      hipLaunchKernelGGL(k_compact, dim3((nBlocks + 3u) / 4u), dim3(256), 0, st, ea.slots, stride, (const uint64_t *)offsets, payload, nBlocks);
    break;
  }
  default:   // ENC_RING_CHUNKS
  {
    // chunk k: encode + size scan on the caller's stream, compaction on the second stream; the slot buffer of chunk k is free again when
    // the compaction of chunk k - 2 is done
    const hipStream_t aux = aux_stream();
    hipEvent_t scanned = nullptr, compacted[2] = { nullptr, nullptr };
    bool ok = aux != nullptr && hipEventCreateWithFlags(&scanned, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&compacted[0], hipEventDisableTiming) == hipSuccess &&
              hipEventCreateWithFlags(&compacted[1], hipEventDisableTiming) == hipSuccess;
    for (uint64_t k = 0; k < w.nChunks && ok; k++)
    {
      const uint64_t first = k * w.chunk;
      const uint32_t count = (uint32_t)((w.nBlocks - first) < w.chunk ? (w.nBlocks - first) : w.chunk);
      uint8_t *slots = ws + w.offSlots + (k & 1u) * w.chunk * (uint64_t)stride;
      if (k >= 2) ok = hipStreamWaitEvent(st, compacted[k & 1u], 0) == hipSuccess;
      EncodeArgs ea{ (const uint8_t *)dIn + first * B, U - first * B, B, count, slots, stride, sizes + first };
      ok = ok && g_launch[codec].enc(ea, st) == hipSuccess && scan_sizes(sizes + first, count, offsets + first, ws, w.levels, st, k ? offsets + first : nullptr) == hipSuccess &&
           hipEventRecord(scanned, st) == hipSuccess && hipStreamWaitEvent(aux, scanned, 0) == hipSuccess;
      if (!ok) break;
      hipLaunchKernelGGL(k_compact, dim3((count + 3u) / 4u), dim3(256), 0, aux, (const uint8_t *)slots, stride, (const uint64_t *)(offsets + first), payload, count);
      ok = hipEventRecord(compacted[k & 1u], aux) == hipSuccess;
    }
    // the caller's stream continues when every compaction is done
    ok = ok && hipStreamWaitEvent(st, compacted[0], 0) == hipSuccess && hipStreamWaitEvent(st, compacted[1], 0) == hipSuccess;
    if (scanned) (void)hipEventDestroy(scanned);
    if (compacted[0]) (void)hipEventDestroy(compacted[0]);
    if (compacted[1]) (void)hipEventDestroy(compacted[1]);
    if (!ok) rc = HSRLE_ERR_DEVICE;
  }
  }
  if (rc == HSRLE_OK && !finished)
  {
    hipLaunchKernelGGL(k_finish_container, dim3(1), dim3(64), 0, st, container, (uint32_t)codec, U, B, nBlocks);
    if (hipGetLastError() != hipSuccess) rc = HSRLE_ERR_DEVICE;
  }
  scratch_free(own, st);
  return rc;
}

static int check_info(const ContainerHeader &h, uint64_t containerSize, hsrle_container_info_t *info)
{
  static const char m[8] = { 'H', 'S', 'R', 'L', 'E', 'K', 'I', 'T' };
  if (memcmp(h.magic, m, 8) != 0 || h.version != 1 || h.codec >= (uint32_t)kCodecCount)
    return HSRLE_ERR_FORMAT;
  if (!valid_block_size(h.blockSize) || h.uncompressedSize == 0)
    return HSRLE_ERR_FORMAT;
  if (h.blockCount != block_count(h.uncompressedSize, h.blockSize))
    return HSRLE_ERR_FORMAT;
  const uint64_t payloadStart = HSRLE_CONTAINER_HEADER_SIZE + 8ull * ((uint64_t)h.blockCount + 1ull);
  if (h.totalSize != payloadStart + h.payloadSize + HSRLE_CONTAINER_TAIL_PAD || h.totalSize > containerSize)
    return HSRLE_ERR_FORMAT;
  info->version = h.version;
  info->codec = h.codec;
  info->uncompressedSize = h.uncompressedSize;
  info->blockSize = h.blockSize;
  info->blockCount = h.blockCount;
  info->payloadSize = h.payloadSize;
  info->totalSize = h.totalSize;
  return HSRLE_OK;
}

// THE prologue of the decode entry points: the argument checks in their observable order (hsrle_codecs.h: a null pointer beats a bad info, which beats a bad range, which
// beats the capacity), then the device, then the launch arguments.  HSRLE_OK with count == 0: nothing to launch -- the entry returns it, behind the device check.
static int decode_prologue(const void *dContainer, const hsrle_container_info_t *info, uint32_t first, uint32_t count, void *dOut, uint64_t cap, uint32_t *dStatus, DecodeArgs *da)
{
  int rc = decode_info_check(dContainer, info, dOut);
  if (rc == HSRLE_OK) rc = decode_range_check(*info, first, count, cap);
  if (rc != HSRLE_OK)
    return rc;
  if (!device_ok())
    return HSRLE_ERR_DEVICE;
  init_tables();
  const uint8_t *container = (const uint8_t *)dContainer;
  const uint8_t *payload = container + HSRLE_CONTAINER_HEADER_SIZE + 8ull * ((uint64_t)info->blockCount + 1ull);
  *da = DecodeArgs{ payload, (const uint64_t *)(container + HSRLE_CONTAINER_HEADER_SIZE), payload + info->payloadSize + HSRLE_CONTAINER_TAIL_PAD,
                    (uint8_t *)dOut, info->uncompressedSize, info->blockSize, first, count, dStatus };
  return HSRLE_OK;
}

static int decompress_blocks_async(const void *dContainer, const hsrle_container_info_t *info, uint32_t first, uint32_t count, void *dOut, uint64_t cap,
                                   uint32_t *dStatus, hipStream_t st)
{
  DecodeArgs da;
  const int rc = decode_prologue(dContainer, info, first, count, dOut, cap, dStatus, &da);
  if (rc != HSRLE_OK || count == 0)
    return rc;
  if (!g_launch[info->codec].dec)
    return HSRLE_ERR_UNSUPPORTED;
  return g_launch[info->codec].dec(da, st) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

// ------------------------------------------------------------------------------------------------------------------
// split decode of a container: every block is cut into sub-blocks of SB output bytes.  One lane per block walks the block's packets
// (k_container_records) and leaves the decoder state at every SB bytes; the block kernel then runs one lane per SUB-block.  For
// containers with too few blocks to fill the GPU with one lane per block (an 88 MB frame in 4 KiB blocks has 21 600): the block size,
// and with it the compression ratio, stays what it is.

constexpr uint32_t kPacketListBelow = 81920u;     // blocks: up to here the packet list decode is the library's choice for small containers
static uint32_t split_sub_block(const hsrle_container_info_t *info, uint32_t want)
{
  const uint32_t B = info->blockSize;
  // the packet-list decode (hsrle_index.hip.h: k_container_packets, hsrle_expand.hip.h): the library's choice for blocks of up to 16 KiB --
  // the 88 MB frame: 102 us against 180 with records at every 1 KiB and 322 with one lane per block.  It wins up to ~65 536 blocks (256 MiB
  // in 4 KiB blocks: 183 / 186 us video-shaped rle64_3symlut_byte / run-distributed rle8_packed against 329 / 212 plain) and loses at 131 072
  // (408 / 591 against 361 / 274): from 81 920 blocks on one lane per block has the waves it needs.  Records were never the fastest of the
  // three at any size (experiments/r04/call24.sh); they remain for blocks above 16 KiB, whose offsets do not fit the list entries.
  const bool listFits = B <= kPacketListMaxBlock && B >= 256u;
  if (want == HSRLE_SPLIT_PACKET_LIST)
    return listFits ? HSRLE_SPLIT_PACKET_LIST : B;
  if (want == 0u && listFits)
    return info->blockCount <= kPacketListBelow ? HSRLE_SPLIT_PACKET_LIST : B;
  if (want == 0u)
  {
    want = pow2_floor(info->uncompressedSize >> 16);                 // ~2^16 .. 2^17 lanes (measured on the 88 MB frame: 1 KiB sub-blocks 187 us, 512 / 256 bytes 206)
    want = want < 256u ? 256u : want;
  }
  if (want >= B || (want % 128u) != 0u || (B % want) != 0u)
    return B;                                                           // no split
  return want;
}

static int decompress_split_async(const void *dContainer, const hsrle_container_info_t *info, uint32_t first, uint32_t count, void *dOut, uint64_t cap, uint32_t *dStatus,
                                  void *dWs, uint64_t wsSize, uint32_t subBlock, hipStream_t st)
{
  // (no split -> the plain decode: decided on a good info, before the range and the capacity are looked at)
  int rc = decode_info_check(dContainer, info, dOut);
  if (rc != HSRLE_OK)
    return rc;
  const uint32_t SB = split_sub_block(info, subBlock);
  if (SB == info->blockSize)
    return decompress_blocks_async(dContainer, info, first, count, dOut, cap, dStatus, st);
  DecodeArgs da;
  rc = decode_prologue(dContainer, info, first, count, dOut, cap, dStatus, &da);
  if (rc != HSRLE_OK || count == 0)
    return rc;
  if (!g_launch[info->codec].dec || !g_launch[info->codec].sub)
    return HSRLE_ERR_UNSUPPORTED;

  if (SB == HSRLE_SPLIT_PACKET_LIST)
  {
    const uint64_t countsBytes = packet_list_counts_bytes(count);
    if (dWs == nullptr || ((uintptr_t)dWs & 15u) != 0u || wsSize < countsBytes + (uint64_t)count * packet_list_cap(info->blockSize) * 8ull)
      return HSRLE_ERR_CAPACITY;
    if (g_launch[info->codec].sub(da, kSubPacketList, (uint32_t *)dWs, st) != hipSuccess)
      return HSRLE_ERR_DEVICE;
    return launch_expand_packets(kCodecs[info->codec].S, da, (const uint64_t *)((const uint8_t *)dWs + countsBytes), (const uint32_t *)dWs, st) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
  }

  const uint32_t per = info->blockSize / SB;
  const uint64_t subFirst = (uint64_t)first * per;
  const uint64_t subAll = (info->uncompressedSize + SB - 1u) / SB;
  uint64_t subEnd = ((uint64_t)first + count) * per;
  if (subEnd > subAll) subEnd = subAll;
  if (subEnd - subFirst > 0xFFFFFFF0ull || subEnd > 0xFFFFFFF0ull)
    return HSRLE_ERR_ARGUMENT;
  if (dWs == nullptr || wsSize < (subEnd - subFirst) * 4ull * kEntryRecDwords)
    return HSRLE_ERR_CAPACITY;

  // records are indexed by the global sub-block number: hand the kernel the address record 0 would have
  uint32_t *rec0 = (uint32_t *)((uintptr_t)dWs - (uintptr_t)(subFirst * 4ull * kEntryRecDwords));
  if (g_launch[info->codec].sub(da, SB, rec0, st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  da.B = SB; da.firstBlock = (uint32_t)subFirst; da.blockCount = (uint32_t)(subEnd - subFirst);
  da.entries = (const uint32_t *)dWs; da.entryBase = (uint32_t)subFirst;
  return g_launch[info->codec].dec(da, st) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

// one WAVE per block (experiments/hsrle_decode_wave.hip.h): for containers with too few blocks to fill the chip with one lane each
constexpr uint32_t kWaveDecodeBelow = 65536u;     // blocks: above, one lane per block has the waves it needs
static int decompress_wave_async(const void *dContainer, const hsrle_container_info_t *info, uint32_t first, uint32_t count, void *dOut, uint64_t cap, uint32_t *dStatus, hipStream_t st)
{
  int rc = decode_info_check(dContainer, info, dOut);
  if (rc != HSRLE_OK)
    return rc;
  if (info->blockSize > 16384u || !kExperiments)                        // (the wave-per-block decoder is not part of the shipped build: measured slower than the split decode)
    return HSRLE_ERR_UNSUPPORTED;
  DecodeArgs da;
  rc = decode_prologue(dContainer, info, first, count, dOut, cap, dStatus, &da);
  if (rc != HSRLE_OK || count == 0)
    return rc;
  if (!g_launch[info->codec].sub)
    return HSRLE_ERR_UNSUPPORTED;
  return g_launch[info->codec].sub(da, 0u, nullptr, st) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;     // (sub-block size 0 = the wave decoder)
}

} // namespace hsrle
