// hsrle_launch.h -- host-side launch table: codec id -> kernel launchers (CodecLaunch).  The kernels are instantiated per symbol
// width in inst_w*.hip (one translation unit per width so the library builds in parallel).
#pragma once
#include <atomic>

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "hsrle_codecs.h"
#include "hsrle_ring_probe.hip.h"

namespace hsrle {

// Developer knobs (A/B runs, forcing a kernel variant in the parity suite) exist only in -DHSRLE_EXPERIMENTS builds (tools/build_variant.sh
// exp -DHSRLE_EXPERIMENTS): the shipped library reads no environment variable in any launch path and holds one kernel per codec and case.
#ifdef HSRLE_EXPERIMENTS
inline uint32_t knob_u32(const char *name, uint32_t dflt) { const char *e = getenv(name); return (e && *e) ? (uint32_t)strtoul(e, nullptr, 10) : dflt; }
constexpr bool kExperiments = true;
#else
constexpr uint32_t knob_u32(const char *, uint32_t dflt) { return dflt; }
constexpr bool kExperiments = false;
#endif

struct DecodeArgs
{
  const uint8_t *payload;
  const uint64_t *offsets;
  const uint8_t *payloadEnd; // payload + payloadSize + tail pad: last readable byte + 1
  uint8_t *out;
  uint64_t U;
  uint32_t B, firstBlock, blockCount;
  uint32_t *status;
  int *residentWorkgroups = nullptr; // query mode: no launch; receives the number of workgroups (= waves) of this kernel that fit on one CU
  const uint32_t *entries = nullptr; // lane b starts from entry record b - entryBase (hsrle_index.hip.h) instead of from a block stream header
  uint32_t entryBase = 0;
  const uint32_t *gate = nullptr;    // decode enqueued BEFORE the host has seen the index passes' verdict: gate[0] | gate[1] != 0 (regions to repair / malformed) -> the kernel returns at once
  uint32_t gateWords = 2;            // words of the gate: 2 (the resolve pass's verdict) or 1 (the range decode's status word)
  uint64_t winLo = 0, winHi = ~0ull; // output window: position p is stored at out + (p - winLo) iff winLo <= p < winHi (range decode); the lanes still decode whole blocks
};

// index passes over one monolithic stream (hsrle_index.hip.h)
struct IndexArgs
{
  const uint8_t *stream;        // device pointer to the stream's first byte (>= 64 readable bytes in front, >= 64 behind)
  uint32_t C, p0, G, M, R;      // stream bytes, first packet, region size, look-back of the guess, regions
  uint32_t single, singleSym;   // 8 bit Single mode / rle8_single_short: mode flag and the stream's one symbol
  const uint32_t *list; uint32_t listCount; const uint32_t *fix;   // repair pass: regions to walk again and their true entries
  uint32_t *mark; uint32_t roundTag; uint32_t extMax;                           //              mark[r] == roundTag: region r is on this round's list
  uint32_t *g, *e; uint64_t *olen; uint32_t *t;                       // walk results per region
  const uint32_t *entry; const uint64_t *outStart; const uint32_t *stateIn; uint64_t U; uint32_t B; uint32_t *rec;   // record pass
  const uint32_t *gate = nullptr;   // record pass enqueued BEFORE the host has seen the resolve verdict: gate[0] | gate[1] != 0 (regions to repair / malformed) -> writes nothing
};
typedef hipError_t (*IndexLaunch)(const IndexArgs &, int records, hipStream_t);
// container blocks cut into sub-blocks of SB output bytes: entry records for [firstBlock, firstBlock + blockCount) of `a` into rec
typedef hipError_t (*SubBlockLaunch)(const DecodeArgs &a, uint32_t SB, uint32_t *rec, hipStream_t);

struct EncodeArgs
{
  const uint8_t *in;
  uint64_t U;
  uint32_t B, nBlocks;
  uint8_t *slots;
  uint32_t slotStride;
  uint32_t *sizes;
  int *residentWorkgroups = nullptr; // query mode, as in DecodeArgs
  uint32_t *ringSel = nullptr;       // 16 bytes of device scratch: the encoders of 1 / 2 byte symbols choose their history ring per input (hsrle_encode8.hip.h)
};

// chunks of ONE monolithic stream (hsrle_mono_encode.hip.h): EncodeArgs with nBlocks = chunks, plus the chunk table
struct MonoEncodeArgs
{
  const uint64_t *starts; uint64_t *syms; const uint64_t *slotOff; uint32_t steps;   // (syms: rewritten by k_encodeS_blocks when it settles the lists itself)
  uint64_t *listOut = nullptr; uint32_t dry = 0;     // codecs with a move-to-front list: syms / listOut hold 8 words per chunk
  const uint32_t *pick = nullptr;                    // 8 bit Single: the stream's symbol (device); split encode of a container: a BYTE per block
  uint32_t phase = 0;                                // split encode, Single codecs: 1 = only pick the blocks' symbols into `pick` -- and find the blocks' cuts:
  uint64_t *cutPos = nullptr, *cutSym = nullptr; uint32_t *cutFlags = nullptr; uint32_t cutG = 0, cutLong = 0;   // (phase 1) per piece of cutG bytes, as k_mono_cuts8 leaves them
  uint64_t *jobs = nullptr; uint32_t *jobCount = nullptr; uint32_t jobCap = 0;   // 8 bit Single: literal stretches noted for k_copy_jobs
};
typedef hipError_t (*MonoEncodeLaunch)(const EncodeArgs &, const MonoEncodeArgs &, hipStream_t);
// wave-per-block encoder (hsrle_encode8w.hip.h): writes offsets and payload of the container directly
struct WaveEncodeArgs
{
  const uint8_t *in; uint64_t U; uint32_t B, nBlocks;
  uint64_t *offsets; uint8_t *payload;
  unsigned long long *tiles; uint32_t *ticket;      // zeroed by the caller: one word per block, one counter
  int *residentWorkgroups = nullptr;                // query mode
};
typedef hipError_t (*WaveEncodeLaunch)(const WaveEncodeArgs &, hipStream_t);
// position-parallel encoder (hsrle_encode8p.hip.h): phase 0 = sizes[] and the blocks' records, phase 1 = -- behind the caller's scan -- the streams at
// payload + offsets[b].  scratch: pp_scratch_bytes(nBlocks), 256-byte aligned; it needs no initialisation
struct PpArgs
{
  const uint8_t *in; uint64_t U; uint32_t B, nBlocks;
  uint32_t *sizes; const uint64_t *offsets; uint8_t *payload; uint8_t *scratch;
};
inline uint32_t pp_record_stride(uint32_t B) { return B / 4u < kPpRecords ? B / 4u : kPpRecords; }      // (4 * stride + 4 bytes per block: less than a staging slot of B + 193)
inline uint64_t pp_scratch_bytes(uint64_t nBlocks, uint32_t B) { return (4ull * pp_record_stride(B) + 4ull) * nBlocks + 256ull; }
typedef hipError_t (*PpLaunch)(const PpArgs &, int phase, hipStream_t);
// the same encoder for units of any length, window by window (hsrle_encode8pw.hip.h): phase 0 = one wave per unit (sizes[], window states, records),
// phase 1 = one wave per window (the packets of the runs that end in it)
constexpr uint32_t kPpwWindow = kPpMaxBlock;                    // bytes per window
constexpr uint32_t kPpwStateWords = 8u;                          // per window: posW, lastRLE, openStart, lastSymbol, stored runs, unit, window in unit, -
constexpr uint32_t kPpwEmpty = 0xFFFFFFFEu;                      // state word 4: no such window
constexpr uint32_t kPpwStride = kPpRecords;                      // records per window

struct PpwArgs
{
  const uint8_t *in; uint64_t U;
  uint32_t B;                     // != 0: the units are the blocks of a container (header + terminator each); 0: the chunks of ONE stream (no header, the last one ends it)
  uint32_t nUnits;                // blocks / an upper bound of the chunks
  const uint64_t *starts;         // chunks: [count + 1] input positions
  const uint64_t *syms;           // chunks: lastSymbol in front of each
  const uint32_t *count;          // chunks: how many there are (device)
  uint32_t *sizes; const uint64_t *offsets; uint8_t *payload;
  uint32_t *states;               // [nWindows][kPpwStateWords]
  uint32_t *recs;                 // [nWindows][kPpwStride]
  uint32_t nWindows;
  uint32_t *fail;                 // chunks of the 1 .. 8 byte symbol codecs (hsrle_encodeSpw.hip.h): set to 1 by a chunk that did not end on its boundary run
};
inline uint64_t ppw_scratch_bytes(uint64_t nWindows) { return nWindows * (4ull * kPpwStateWords + 4ull * kPpwStride) + 512ull; }

typedef hipError_t (*PpwLaunch)(const PpwArgs &, int phase, hipStream_t);
constexpr uint32_t kPpwLStateWords = 32u;                        // ... of the general LUT kernel's (hsrle_encodeLpw.hip.h): the list travels in the state record
constexpr uint32_t kPpwSStateWords = 16u;                        // ... of the 1 .. 8 byte symbol codecs' windowed encoder (hsrle_encodeSpw.hip.h): more state crosses a window's edge
                                                                 // (word 12 = the stored runs: kPpwEmpty there marks a slot with no such window)
typedef hipError_t (*DecodeLaunch)(const DecodeArgs &, hipStream_t);
typedef hipError_t (*EncodeLaunch)(const EncodeArgs &, hipStream_t);

constexpr uint32_t kEncodeLdsCap = 20000;       // bytes of dynamic LDS per encode workgroup (0 = no residency cap); tuned on MI355X
#ifndef HSRLE_DECODE_TILE
#define HSRLE_DECODE_TILE 128
#endif
#ifndef HSRLE_DECODE_RING
#define HSRLE_DECODE_RING 128
#endif
#ifndef HSRLE_DECODE_STEP
#define HSRLE_DECODE_STEP 128
#endif
constexpr int kDecodeStep = HSRLE_DECODE_STEP; // output bytes per lane and decode/top-up step (k_decode_blocks Q)
constexpr int kDecodeTile = HSRLE_DECODE_TILE; // bytes produced per lane and round (k_decode_blocks T)
constexpr int kDecodeRing = HSRLE_DECODE_RING; // per-lane stream ring in LDS (k_decode_blocks R)

// the 8 bit list-free (plain / Packed) decoders' tile row, step and ring (A/B builds: -DHSRLE_DEC8_TILE=64 -DHSRLE_DEC8_STEP=64)
#ifndef HSRLE_DEC8_TILE
#define HSRLE_DEC8_TILE HSRLE_DECODE_TILE
#endif
#ifndef HSRLE_DEC8_STEP
#define HSRLE_DEC8_STEP HSRLE_DECODE_STEP
#endif
#ifndef HSRLE_DEC8_RING
#define HSRLE_DEC8_RING HSRLE_DECODE_RING
#endif
constexpr int kDec8Tile = HSRLE_DEC8_TILE, kDec8Step = HSRLE_DEC8_STEP, kDec8Ring = HSRLE_DEC8_RING;
// the A/B build knobs of the decode rule (hsrle_codecs.h: decode_variant) and of the encoders of 2 .. 8 byte symbols (hsrle_inst_generic.inc)
#ifdef HSRLE_DECODE_ALWAYS_ENT
constexpr bool kDecodeAlwaysEnt = true;
#else
constexpr bool kDecodeAlwaysEnt = false;
#endif
#ifdef HSRLE_DEC8_PE
constexpr bool kDec8Pe = true;
#else
constexpr bool kDec8Pe = false;
#endif
constexpr DecodeKnobs kDecodeKnobs{ kDecodeAlwaysEnt, kDec8Pe };
#ifdef HSRLE_ENCODE_V1   // the first-generation encoder (per-lane global reads and writes, hsrle_encode.hip.h)
constexpr bool kEncodeV1 = true;
#else
constexpr bool kEncodeV1 = false;
#endif
#ifdef HSRLE_ENCS_RING   // one history ring for every width (hsrle_encodeS.hip.h)
constexpr bool kEncSRingFixed = true;
#else
constexpr bool kEncSRingFixed = false;
#endif

// One row per codec id: every launcher the codec has (nullptr: none).  The inst_*.hip units fill their columns (register_*), hsrle_capi_host.h owns the table.
struct CodecLaunch
{
  DecodeLaunch dec; EncodeLaunch enc; IndexLaunch idx; SubBlockLaunch sub; MonoEncodeLaunch menc;
  WaveEncodeLaunch wenc;   // experiment builds: rle8_multi, rle8_packed_multi
  PpLaunch pp;             // position-parallel encoder, blocks up to 4 KiB
  // the windowed position-parallel encoders, blocks above 4 KiB: rle8_multi / rle8_packed_multi (hsrle_encode8pw.hip.h, also the chunks of their monolithic streams),
  // the codecs of hsrle_encodeLp.hip.h, those of hsrle_encodeSp.hip.h -- and the latter's chunk mode (the chunks of one monolithic stream): the 42 codecs the cut fixes the state of
  PpwLaunch ppw8, ppwL, ppwS, ppwSM;
};
void register_w8(CodecLaunch *t);
void register_w16(CodecLaunch *t);
void register_w24(CodecLaunch *t);
void register_w32(CodecLaunch *t);
void register_w48(CodecLaunch *t);
void register_w64(CodecLaunch *t);
void register_w128(CodecLaunch *t);
void register_pp8(CodecLaunch *t);
void register_pp8s(CodecLaunch *t);
void register_pp128(CodecLaunch *t);
void register_ppL(CodecLaunch *t);
void register_ppS(CodecLaunch *t);
void register_pp8w(CodecLaunch *t);
void register_ppLw(CodecLaunch *t);
void register_ppSw(CodecLaunch *t);    // ppwS and ppwSM

// the scratch of a position-parallel launch as its kernels take it (PpScratch: hsrle_encode8p.hip.h)
struct PpScratch;
template <typename SCRATCH = PpScratch>
inline SCRATCH pp_scratch_of(const PpArgs &a)
{
  SCRATCH sc;
  sc.recs = (uint32_t *)a.scratch;
  sc.recStride = pp_record_stride(a.B);
  sc.recCount = sc.recs + (uint64_t)sc.recStride * a.nBlocks + 64u;   // (+ 64: the last block's lanes read 64 words from its first record on)
  sc.stamps = nullptr;
  return sc;
}

template <typename... A>
constexpr int kernel_arity(void (*)(A...)) { return (int)sizeof...(A); }

// a launch with an output window other than [0, U) (range decode) takes the kernel instantiation with the window code (k_decode_blocks WIN)
inline bool windowed(const DecodeArgs &a) { return a.winLo != 0ull || a.winHi < a.U; }

template <typename KERNEL>
inline hipError_t launch_decode(KERNEL k, const DecodeArgs &a, hipStream_t st)
{
  if (a.residentWorkgroups != nullptr)
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(a.residentWorkgroups, k, 64, 0);
  const uint32_t grid = (a.blockCount + 63u) / 64u;
  hipLaunchKernelGGL(k, dim3(grid), dim3(64), 0, st, a.payload, a.offsets, a.payloadEnd, a.out, a.U, a.B, a.firstBlock, a.blockCount, a.status, a.entries, a.entryBase, a.gate, a.gateWords, a.winLo, a.winHi);
  return hipGetLastError();
}

// Decoders: containers whose streams shrink to less than a quarter (1 / 2 byte symbols) or a fifth take the instantiation with a 64-byte
// stream ring (12 instead of 9 waves per CU; a lane rarely needs more than 64 stream bytes for 128 output bytes there, and one that
// does finishes in the second pass).  8 GiB video-shaped rle8_packed (ratio 0.18): 3.90 -> 3.34 ms; at ratio 0.43 it would lose 9 %,
// on run-distributed data 9 - 25 %.  Blocks decoded from entry records (monolithic streams, split decode) keep the 128-byte ring.
// HSRLE_DEC_RING=64 / 128 in the environment forces one (tests, A/B; experiment builds).
// THE predicate: launch_decode_codec below and hsrle_decode_ring (include/hsrle.h) both ask it, with the codec's threshold from its row (hsrle_codecs.h:
// small_ring_per_mille; a codec without a 64-byte instantiation never takes one, forced or not).  readableBytes = payloadSize + the tail pad.
inline bool decode_ring_small(const CodecInfo &c, uint64_t U, uint64_t readableBytes)
{
  static const int forced = (int)knob_u32("HSRLE_DEC_RING", 0);
  const uint64_t perMille = small_ring_per_mille(c);
  if (perMille == 0u) return false;
  return forced ? forced == 64 : readableBytes * 1000u < U * perMille;
}
// The block decoder (hsrle_decode.hip.h; declared here so that the launcher below stands in a header the C-ABI unit reads too)
template <int FAM, int S, int AL, int T, int R, int Q, bool SGL, bool ENT, bool WIN>
__global__ void k_decode_blocks(const uint8_t *__restrict__ payload, const uint64_t *__restrict__ offsets, const uint8_t *__restrict__ payloadEnd, uint8_t *__restrict__ out, uint64_t U,
                                uint32_t B, uint32_t firstBlock, uint32_t blockCount, uint32_t *__restrict__ status, const uint32_t *__restrict__ entries, uint32_t entryBase,
                                const uint32_t *__restrict__ gate, uint32_t gateWords, uint64_t winLo, uint64_t winHi);
#ifdef HSRLE_DEC8_PE   // ... and the experiment's (csrc/experiments/hsrle_decode8pe.hip.h)
template <int FAM>
__global__ void k_decode8_pe(const uint8_t *__restrict__ payload, const uint64_t *__restrict__ offsets, const uint8_t *__restrict__ payloadEnd, uint8_t *__restrict__ out, uint64_t U,
                             uint32_t B, uint32_t firstBlock, uint32_t blockCount, uint32_t *__restrict__ status, const uint32_t *__restrict__ entries, uint32_t entryBase,
                             const uint32_t *__restrict__ gate, uint32_t gateWords, uint64_t winLo, uint64_t winHi);
#endif

// one case of the rule (hsrle_codecs.h: decode_variant) for codec id C: the kernel it names.  Cases with the same answer are the same kernel.
template <int C, bool WINDOW, bool ENTRIES, bool SMALL>
inline hipError_t launch_decode_case(const DecodeArgs &a, hipStream_t st)
{
  constexpr DecodeVariant v = decode_variant(kCodecs[C], WINDOW, ENTRIES, SMALL, kDecodeKnobs);
  constexpr int S = kCodecs[C].S, AL = kCodecs[C].aligned, T = v.list8 ? kDec8Tile : kDecodeTile, Q = v.list8 ? kDec8Step : kDecodeStep;
  constexpr int R = v.ring == 64 ? 64 : (v.list8 ? kDec8Ring : kDecodeRing);
#ifdef HSRLE_DEC8_PE
  if constexpr (v.pe) return launch_decode(k_decode8_pe<v.fam>, a, st);
  else
#endif
  return launch_decode(k_decode_blocks<v.fam, S, AL, T, R, Q, v.sgl, v.ent, v.win>, a, st);
}
// THE decode launcher of codec id C: instantiates what the rule can answer for this codec and takes the one it answers for this launch.  A query
// (a.residentWorkgroups) has U == 0 and no entries: it gets the plain container's 128-byte instantiation unless a ring is forced.
template <int C>
inline hipError_t launch_decode_codec(const DecodeArgs &a, hipStream_t st)
{
  if (windowed(a)) return launch_decode_case<C, true, false, false>(a, st);
  if (a.entries != nullptr) return launch_decode_case<C, false, true, false>(a, st);
  if (decode_ring_small(kCodecs[C], a.U, (uint64_t)(a.payloadEnd - a.payload))) return launch_decode_case<C, false, false, true>(a, st);
  return launch_decode_case<C, false, false, false>(a, st);
}

// blocks per wave: all of a small container's waves resident at once.  How many waves of a kernel a CU holds is asked once per kernel
// (LDS and registers decide: 7 .. 10 for the run list encoders) and remembered in a small table; racing first calls write the same value.
inline uint32_t run_list_waves_per_cu(const void *kernel, hipStream_t st)
{
  struct Entry { std::atomic<const void *> k; std::atomic<int> v; };
  static Entry table[256];
  for (auto &e : table)
  {
    const void *have = e.k.load(std::memory_order_acquire);
    if (have == kernel) { const int v = e.v.load(std::memory_order_relaxed); if (v > 0) return (uint32_t)v; break; }
    if (have == nullptr) break;
  }
  // (not hipOccupancyMaxActiveBlocksPerMultiprocessor: it divides the LDS without the 1 280-byte allocation granule and says 11 or 12 where the
  //  hardware holds 10 -- and a grid just above what is resident leaves a tail of waves that run alone: 88 MB frame 215 us instead of 161)
  int n = 8;
  // (a first call that is being captured into a graph asks nothing: the query is not a stream operation, and what may and may not be called
  //  under capture is the runtime's business -- the default serves, the next eager call fills the table)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return (uint32_t)n;
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, kernel) == hipSuccess)
  {
    const uint32_t lds = (((uint32_t)fa.sharedSizeBytes + 1279u) / 1280u) * 1280u, regs = (((uint32_t)fa.numRegs + 7u) / 8u) * 8u;
    const uint32_t byLds = lds ? 163840u / lds : 32u, byRegs = regs ? 4u * (512u / regs > 8u ? 8u : 512u / regs) : 32u;
    n = (int)(byLds < byRegs ? byLds : byRegs);
    if (n < 1) n = 1;
    if (knob_u32("HSRLE_RL_DEBUG", 0u)) fprintf(stderr, "run list kernel %p: lds %zu regs %d -> %d waves per CU\n", kernel, (size_t)fa.sharedSizeBytes, fa.numRegs, n);
  }
  for (auto &e : table)
  {
    const void *expected = nullptr;
    if (e.k.load(std::memory_order_acquire) == kernel || e.k.compare_exchange_strong(expected, kernel)) { e.v.store(n, std::memory_order_relaxed); break; }
  }
  return (uint32_t)n;
}

template <typename KERNEL>
inline hipError_t launch_run_list(KERNEL k, const EncodeArgs &a, hipStream_t st)
{
  const uint32_t resident = 256u * run_list_waves_per_cu((const void *)k, st);
  const uint32_t want = (a.nBlocks + resident - 1u) / resident;
  const uint32_t bpw = knob_u32("HSRLE_RL_BPW", want > 64u ? 64u : want);
  hipLaunchKernelGGL(k, dim3((a.nBlocks + bpw - 1u) / bpw), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.slots, a.slotStride, a.sizes, bpw, (const uint32_t *)nullptr);
  return hipGetLastError();
}

template <typename KERNEL>
inline hipError_t launch_encode(KERNEL k, const EncodeArgs &a, hipStream_t st, int capResidency = 1)
{
  const uint32_t grid = (a.nBlocks + 63u) / 64u;
  // The encoder keeps one 128-byte line per lane open on the read side and one on the write side.  With the full 32 waves per CU
  // those open lines (32 CUs x 32 waves x 64 lanes x 2 x 128 B = 16 MiB per XCD) thrash the 4 MiB L2 and every line is fetched /
  // written several times (measured: 6.8x read, 5.9x write amplification).  A dynamic LDS reservation caps the residency.
  static const uint32_t ldsCap = knob_u32("HSRLE_ENCODE_LDS_CAP", kEncodeLdsCap);
  static const uint32_t lds8 = knob_u32("HSRLE_ENCODE8_LDS", 0u);
  if (a.residentWorkgroups != nullptr)
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(a.residentWorkgroups, k, 64, capResidency ? ldsCap : lds8);
  if constexpr (kernel_arity(KERNEL{}) == 14)   // kernels with a MONO mode (hsrle_encode8.hip.h): block mode = no chunk table
    hipLaunchKernelGGL(k, dim3(grid), dim3(64), capResidency ? ldsCap : lds8, st, a.in, a.U, a.B, a.nBlocks, a.slots, a.slotStride, a.sizes, (const uint64_t *)nullptr,
                       (uint64_t *)nullptr, (const uint64_t *)nullptr, 0u, (uint64_t *)nullptr, 0u, (const uint32_t *)nullptr);
  else
    hipLaunchKernelGGL(k, dim3(grid), dim3(64), capResidency ? ldsCap : lds8, st, a.in, a.U, a.B, a.nBlocks, a.slots, a.slotStride, a.sizes);
  return hipGetLastError();
}

// the encoders of 1 / 2 byte symbols: probe a sample of the input, then both instantiations -- the one that was not chosen returns at once.
// HSRLE_ENC_RING=128 / 256 in the environment forces one (tests, A/B).  Without scratch (a.ringSel == nullptr): the 256-byte ring.
template <int S, typename K256, typename K128>
inline hipError_t launch_encode_ring(K256 k256, K128 k128, const EncodeArgs &a, hipStream_t st)
{
  static const int forced = (int)knob_u32("HSRLE_ENC_RING", 0);
  // (below ~131 072 blocks the device is not full with 9 waves per CU either: more waves bring nothing, and the probe + the second launch
  //  are ~25 us of a call that short)
  if (a.residentWorkgroups != nullptr || forced == 256 || (forced == 0 && (a.ringSel == nullptr || a.nBlocks < 131072u)))
    return launch_encode(k256, a, st, 0);
  if (forced == 128)
    return launch_encode(k128, a, st, 0);
  if (zero_async(a.ringSel, 16, st) != hipSuccess) return hipErrorUnknown;   // (a kernel, not hipMemsetAsync: hsrle_common.hip.h zero_async)
  const uint32_t samples = a.nBlocks < 256u ? a.nBlocks : 256u;
  hipLaunchKernelGGL((k_ring_probe<S>), dim3(samples), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.ringSel);
  hipLaunchKernelGGL((k_ring_decide<S>), dim3(1), dim3(64), 0, st, a.ringSel);
  const uint32_t grid = (a.nBlocks + 63u) / 64u;
  hipLaunchKernelGGL(k256, dim3(grid), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.slots, a.slotStride, a.sizes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint64_t *)nullptr, 0u,
                     (uint64_t *)nullptr, 0u, (const uint32_t *)a.ringSel);
  hipLaunchKernelGGL(k128, dim3(grid), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.slots, a.slotStride, a.sizes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint64_t *)nullptr, 0u,
                     (uint64_t *)nullptr, 0u, (const uint32_t *)a.ringSel);
  return hipGetLastError();
}

#ifdef HSRLE_EXPERIMENTS
template <typename KERNEL>
inline hipError_t launch_wave_encode(KERNEL k, const WaveEncodeArgs &a, hipStream_t st)
{
  static int perCu = 0, cus = 0;
  if (perCu == 0)
  {
    int dev = 0, n = 0, c = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, 64, 0) != hipSuccess ||
        hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0 || c <= 0)
      return hipErrorInvalidValue;
    perCu = n; cus = c;
  }
  if (a.residentWorkgroups != nullptr) { *a.residentWorkgroups = perCu; return hipSuccess; }
  // resident waves take blocks in ticket order
  const uint64_t resident = (uint64_t)perCu * (uint64_t)cus;
  const uint32_t grid = (uint32_t)(a.nBlocks < resident ? a.nBlocks : resident);
  hipLaunchKernelGGL(k, dim3(grid), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.offsets, a.payload, a.tiles, a.ticket);
  return hipGetLastError();
}

#endif

template <typename KERNEL>
inline hipError_t launch_mono_encode(KERNEL k, const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st)
{
  // (a.B != 0: chunks of a container's blocks -- a.ringSel[0] is then the number of chunks: hsrle_encode8.hip.h)
  hipLaunchKernelGGL(k, dim3((a.nBlocks + 63u) / 64u), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.slots, a.slotStride, a.sizes, m.starts, m.syms, m.slotOff, m.steps, m.listOut, m.dry, (const uint32_t *)a.ringSel);
  return hipGetLastError();
}

} // namespace hsrle
