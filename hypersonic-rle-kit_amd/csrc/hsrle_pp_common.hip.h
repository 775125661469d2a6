// hsrle_pp_common.hip.h -- what the position-parallel encoders share (hsrle_encode8p / 8pw / Sp / Spw / Lp / Lpw / 8sp / 128p .hip.h), so that no encoder reaches
// a helper through another family's encoder:
//   * the wave primitives on DPP, the LDS layout of one wave's block (PpShared), the scratch between the two launches (PpScratch);
//   * the input side: pp_load / ppw_load, pp_symbol / ppw_symbol_at, and for symbols of S bytes the run behind a stretch of match bits (pp_shl_in, pp_run_from);
//   * the image side: pp_or_bytes, pp_put_chunks (literals), pp_init_mlut, ppw_img16.
// The rules that one pair of kernels shares stand in the pair's block file: pp8_decide (hsrle_encode8p.hip.h), ppS_decide (hsrle_encodeSp.hip.h).
// A rule that reads several of a round's locals takes them as one small struct of references, built where the rule's lambda used to stand (Pp8Run, PpSRun,
// PpStretch).  That form is deliberate: the compiler treats it like the closure it replaces, and every kernel compiles to the code it had before.
#pragma once

#include "hsrle_common.hip.h"
#include "hsrle_decode.hip.h" // lds_read16, wave_sync

namespace hsrle {

// (kPpMaxBlock, kPpRecords: hsrle_common.hip.h -- the host side needs them too)
constexpr uint32_t kPpNoRecords = 0xFFFFFFFFu;                  // recCount[b]: the block stored more runs than its records hold

// ---- wave-level primitives on DPP (no LDS round trip: a ds_bpermute based __shfl_up costs ~100 cycles of latency per step) ----
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v, uint32_t fill) { return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x138, 0xF, 0xF, false); }   // lane i <- lane i - 1
__device__ __forceinline__ uint32_t wave_shl1(uint32_t v, uint32_t fill) { return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x130, 0xF, 0xF, false); }   // lane i <- lane i + 1
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v)   // inclusive
{
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);
  return v;
}
__device__ __forceinline__ int32_t imax(int32_t a, int32_t b) { return a > b ? a : b; }
__device__ __forceinline__ int32_t wave_scan_max(int32_t v)     // inclusive; values >= -1
{
  v = imax(v, __builtin_amdgcn_update_dpp(-1, v, 0x111, 0xF, 0xF, false));
  v = imax(v, __builtin_amdgcn_update_dpp(-1, v, 0x112, 0xF, 0xF, false));
  v = imax(v, __builtin_amdgcn_update_dpp(-1, v, 0x114, 0xF, 0xF, false));
  v = imax(v, __builtin_amdgcn_update_dpp(-1, v, 0x118, 0xF, 0xF, false));
  v = imax(v, __builtin_amdgcn_update_dpp(-1, v, 0x142, 0xA, 0xF, false));
  v = imax(v, __builtin_amdgcn_update_dpp(-1, v, 0x143, 0xC, 0xF, false));
  return v;
}
__device__ __forceinline__ uint32_t wave_lane(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

constexpr uint32_t kPpCoopMin = 80u;                            // literal stretches longer than this are copied by the whole wave, shorter ones by their packet's lane
constexpr uint32_t kPpJobs = kPpMaxBlock / (kPpCoopMin + 4u) + 2u;
constexpr uint32_t kPpInPad = 16u;                              // the input image starts 16 bytes into its buffer (a literal window may begin up to 15 bytes in front of its stretch)
// LDS of one wave's block
template <bool EMIT, bool INPUT = EMIT, bool MTF = false>
struct PpShared
{
  uint8_t img[EMIT ? (kPpMaxBlock + 193u + 15u + 16u + 15u) / 16u * 16u : 16u] __attribute__((aligned(16)));   // the stream under construction
  uint8_t inb[INPUT ? kPpInPad + kPpMaxBlock + 32u : 16u] __attribute__((aligned(16)));   // the block's input: literals and run symbols come from here, not from L2 (0.8 us per gather under load)
  uint8_t mlut[EMIT ? 17u * 16u : 16u] __attribute__((aligned(16)));   // entry c: the low c bytes, c = 0 .. 16
  uint64_t starts[64];                                                  // run-start bits of every lane's 64 positions
  uint64_t mtfScratch[MTF ? 152u : 1u];                                 // LUT codecs: the round's run symbols and list heads
  uint64_t jobs[EMIT ? kPpJobs : 1u];                                   // literal stretches for the whole wave
  uint16_t lst[64];                                                     // the round's candidates (last byte positions), handed from the lanes that found them to the lanes that judge them
  uint16_t carryStart[64];                                              // start of the run that is open where a lane's positions begin
  uint32_t jobCount;
};

// scratch between the two launches
struct PpScratch
{
  uint32_t *recs;       // [nBlocks][recStride]   start | (end - 1) << 12 | same << 24 | (32 bit range field) << 25, one per stored run
  uint32_t *recCount;   // [nBlocks]              stored runs, kPpNoRecords where they did not fit
  uint32_t recStride;   // pp_record_stride(B)
  uint8_t *stamps;      // diagnostic builds
};

// lane l's 64 bytes of block b (zeros behind the end of the input)
__device__ __forceinline__ void pp_load(const uint8_t *__restrict__ in, uint64_t U, uint32_t B, uint32_t b, u32x4 (&x)[4])
{
  const uint64_t at = (uint64_t)b * B;
  const uint32_t n = (uint32_t)((U - at) < (uint64_t)B ? (U - at) : (uint64_t)B);
  const uint8_t *const d = in + at;
  const uint32_t base = threadIdx.x * 64u;
#pragma unroll
  for (uint32_t j = 0; j < 4u; j++)
  {
    const uint32_t pos = base + 16u * j;
    u32x4 v = u32x4{ 0, 0, 0, 0 };
    if (pos + 16u <= n) v = ld128(d + pos);
    else if (pos < n) v = load16_edge(d, (int64_t)pos, (uint64_t)n);
    x[j] = v;
  }
}

// lane l's 64 bytes of the window at `ws` of a unit of n bytes (zeros behind its end)
__device__ __forceinline__ void ppw_load(const uint8_t *__restrict__ d, uint32_t n, uint32_t ws, u32x4 (&x)[4])
{
  const uint32_t base = ws + threadIdx.x * 64u;
#pragma unroll
  for (uint32_t j = 0; j < 4u; j++)
  {
    const uint32_t pos = base + 16u * j;
    u32x4 v = u32x4{ 0, 0, 0, 0 };
    if (pos + 16u <= n) v = ld128(d + pos);
    else if (pos < n) v = load16_edge(d, (int64_t)pos, (uint64_t)n);
    x[j] = v;
  }
}

// 16 image bytes from any offset (dword reads + a byte funnel: LDS dword reads need no 16-byte alignment)
__device__ __forceinline__ u32x4 ppw_img16(const uint8_t *img, uint32_t off)
{
  const uint32_t *const q = (const uint32_t *)(img + (off & ~3u));
  const uint32_t q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4], sb = off & 3u;
  return u32x4{ alignbyte(q1, q0, sb), alignbyte(q2, q1, sb), alignbyte(q3, q2, sb), alignbyte(q4, q3, sb) };
}

// the S-byte symbol at LDS byte position `at` of the input image (dwords beyond S bytes zero)
template <int S>
__device__ __forceinline__ uint64_t pp_symbol(const uint8_t *inb, uint32_t at)
{
  const uint32_t *const w = (const uint32_t *)(inb + (at & ~3u));
  const uint32_t sb = at & 3u;
  const uint32_t q0 = w[0], q1 = w[1];
  uint32_t lo = alignbyte(q1, q0, sb), hi = 0u;
  if constexpr (S > 4) { const uint32_t q2 = w[2]; hi = alignbyte(q2, q1, sb); }
  if constexpr (S == 1) lo &= 0xFFu;
  if constexpr (S == 2) lo &= 0xFFFFu;
  if constexpr (S == 3) lo &= 0xFFFFFFu;
  if constexpr (S == 6) hi &= 0xFFFFu;
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

// OR the low nb (1 .. 8) bytes of v into the stream image at byte position `at` (LDS atomics on the dwords it touches)
__device__ __forceinline__ void pp_or_bytes(uint8_t *img, uint32_t at, uint64_t v, uint32_t nb)
{
  if (nb < 8u) v &= (1ull << (8u * nb)) - 1ull;
  uint32_t *const wp = (uint32_t *)(img + (at & ~3u));
  const uint32_t sh = 8u * (at & 3u);
  const uint64_t lo = v << sh;
  const uint32_t top = sh ? (uint32_t)(v >> (64u - sh)) : 0u;          // what the shift pushed beyond 64 bits
  atomicOr(wp, (uint32_t)lo);
  if ((uint32_t)(lo >> 32) != 0u) atomicOr(wp + 1, (uint32_t)(lo >> 32));
  if (top != 0u) atomicOr(wp + 2, top);
}

// the merge masks of pp_put_chunks: entry c = the low c bytes (as in k_decode_blocks; entry 16: all of them), by the wave's first 17 lanes
__device__ __forceinline__ void pp_init_mlut(uint8_t *mlut)
{
  if (threadIdx.x < 17u)
  {
    const uint32_t c = threadIdx.x;
    const uint64_t part = ~(~0ull << (8u * (c & 7u)));
    const bool hiHalf = c >= 8u;
    const uint32_t p0 = (c == 16u) ? ~0u : (uint32_t)part, p1 = (c == 16u) ? ~0u : (uint32_t)(part >> 32);
    lds_st128(mlut + c * 16u, u32x4{ hiHalf ? ~0u : p0, hiHalf ? ~0u : p1, hiHalf ? p0 : 0u, hiHalf ? p1 : 0u });
  }
}

// literal bytes [src, src + len) of the block (a window: of the window) -> image bytes [ds, ds + len), the destination chunks t0, t0 + tStep, ... below tEnd of the
// stretch by this lane: a 16-byte window of the input image placed so that every byte lands where it belongs, cut to the stretch under two byte masks, OR-ed into
// the image
template <class SH>
__device__ __forceinline__ void pp_put_chunks(SH &sh, uint32_t src, uint32_t ds, uint32_t len, uint32_t t0, uint32_t tStep, uint32_t tEnd)
{
  const uint32_t de = ds + len, D0 = ds & ~15u;
  for (uint32_t t = t0; t < tEnd; t += tStep)
  {
    const uint32_t D = D0 + 16u * t;
    // (D - ds may be "negative": the pad in front of the image absorbs it.)  Five dwords from the dword below the window + four v_alignbyte: dword
    // reads need no 16-byte alignment, and the 16-byte form (two aligned reads + a select funnel) was 15 vector instructions of the chunk's 35
    const uint32_t wa = kPpInPad + src + D - ds;
    const uint32_t *const wq = (const uint32_t *)(sh.inb + (wa & ~3u));
    const uint32_t q0 = wq[0], q1 = wq[1], q2 = wq[2], q3 = wq[3], q4 = wq[4], sb = wa & 3u;
    const u32x4 v = u32x4{ alignbyte(q1, q0, sb), alignbyte(q2, q1, sb), alignbyte(q3, q2, sb), alignbyte(q4, q3, sb) };
    const uint32_t lo = D < ds ? ds - D : 0u, hi = de - D < 16u ? de - D : 16u;      // chunk bytes [lo, hi)
    const u32x4 mh = lds_ld128(sh.mlut + (hi << 4)), ml = lds_ld128(sh.mlut + (lo << 4));
    unsigned long long *const ip = (unsigned long long *)(sh.img + D);
    const uint64_t w0 = (uint64_t)(v.x & mh.x & ~ml.x) | ((uint64_t)(v.y & mh.y & ~ml.y) << 32), w1 = (uint64_t)(v.z & mh.z & ~ml.z) | ((uint64_t)(v.w & mh.w & ~ml.w) << 32);
    atomicOr(ip, w0);
    atomicOr(ip + 1, w1);
  }
}

// ---- symbols of S bytes (hsrle_encodeSp / Spw / Lp / Lpw .hip.h): the run behind a stretch of match bits ----

// v shifted up by t bits (t < 32) across the wave: the bits that come in from the lane in front are taken from its top dword; `hist`: what comes into lane 0
// (a block: nothing; a window: the match bits in front of it, in the top byte of a dword)
__device__ __forceinline__ uint64_t pp_shl_in(uint64_t v, uint32_t t, uint32_t hist)
{
  const uint32_t top = wave_shr1((uint32_t)(v >> 32), hist);
  return (v << t) | (uint64_t)(top >> (32u - t));
}

// a candidate: the stretch of match bits m[j] = (d[j] == d[j + S]) that starts at s0 and ends in front of position q; nEnd: where the input ends.
// p / e: the run it gives (e == 0: none).  (Member order = the order in which pp_run_from first uses them, as the lambda it replaces captured them: another order
// gives the same results and other device code -- 108 of 110 kernels of inst_ppS.hip moved when it was tried.  Reorder or add members only together with
// tools/device_code_diff.py.)
struct PpStretch { const uint32_t &s0; uint32_t &p, &e; const bool &have; const uint32_t &q, &nEnd; };

// (p, e) of the stretch's run when the reference's scan resumes at `resume` (the end of the run before): it starts at the first position >= resume inside the
// stretch with S bits left, takes whole symbols while they repeat and -- byte-aligned codecs (AL == 0), while a whole symbol would still fit in front of the end
// of the input -- the matching leading bytes of the next one
template <int S, int AL>
__device__ __forceinline__ void pp_run_from(const PpStretch &c, uint32_t resume)
{
  constexpr uint32_t SU = (uint32_t)S;
  const uint32_t ps = resume > c.s0 ? resume : c.s0;
  c.p = ps; c.e = 0u;
  if (c.have && c.q >= ps + SU)
  {
    const uint32_t Leff = c.q - ps;
    const uint32_t whole = ((Leff + SU) / SU) * SU;
    const uint32_t eW = ps + whole;
    c.e = (!AL && eW + SU <= c.nEnd) ? c.q + SU : eW;
  }
}

// the S-byte symbol of the run that starts at p (absolute) and reaches into the window at ws: where the run began more than 16 bytes in front of the window (the
// image holds no more), from a later period of it -- its pattern repeats every S bytes.  (ws by reference on purpose: by value the results are the same and
// 40 of 62 / 116 of 194 windowed kernels compile to other code -- tools/device_code_diff.py.)
template <int S, class SH>
__device__ __forceinline__ uint64_t ppw_symbol_at(SH &sh, const uint32_t &ws, uint32_t p)
{
  constexpr uint32_t SU = (uint32_t)S;
  uint32_t a = p;
  if (ws >= 16u && p < ws - 16u) a = p + ((ws - 16u - p + SU - 1u) / SU) * SU;
  return pp_symbol<S>(sh.inb, kPpInPad + a - ws);
}

} // namespace hsrle
