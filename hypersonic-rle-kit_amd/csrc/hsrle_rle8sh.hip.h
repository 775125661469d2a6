// hsrle_rle8sh.hip.h -- the rle8_sh codec of the reference (src/rle_sh.c, src/rle.h:455-458) for gfx950.
//
// Stream: u32 inSize, u32 streamSize, a BODY of whole bytes that grows upward from offset 8 and a BIT STREAM that grows downward from the last byte:
// bit k of the bit stream is bit k % 8 of byte streamSize - 1 - k / 8.  Tokens are a capped unary code, read LSB first:
//   Z  0       the run symbol R            S  110    `second`                  FILL small  11110    body u8 + 14 bytes of R
//   L  10      one body byte               T  1110   `third`                   and, behind five ones, two type bits:
//   00 raw COPY small (body u8 + 7 bytes)   10 raw COPY large (body u32 + 7 bytes; a stored 0 ENDS the stream)
//   01 FILL large (body u32, then the new R; count = (uint32_t)(stored + 14): the wrap is part of the format)
//   11 ENCODED COPY (body u8 + 161 symbols follow, coded Z / L / S and T as 111)
// Start: R = 0x7F, lastOccurred = 0x80, second = 0x80, third = 0x7E.  A literal equal to lastOccurred promotes (third = second, second = literal);
// every L / S / T makes its own output lastOccurred.
//
// Two properties carry the design:
//  1. TOKENISING NEEDS NO SYMBOL STATE.  Outside an encoded copy every symbol token ends at a zero bit, so a stretch of symbol tokens ends at the
//     first 1-run of length >= 4; it holds as many symbols as zero bits and as many literals as 1-runs of length exactly 1: a few bit operations per
//     64-bit word.
//  2. Only second / third / lastOccurred are carried from token to token, and only L / S / T touch them.
//
//   k_sh_walk          ONE wave tokenises: the bit stream (byte-reversed, so that it reads upward) and the body staged through LDS windows.  Outside
//                      encoded copies it advances by words of the bit stream; it loops per token only inside an encoded copy and at block tokens.
//                      One record per FILL (R), raw COPY (body offset) and symbol stretch (bit offset, body offset, mode, R); a record's length is
//                      the distance to the next record's output offset.  A stretch is cut when it would pass `cap` symbols, so a record is bounded
//                      work for one lane.  EVERY malformed verdict comes from here, before anything is written to the output.
//   k_sh_state         the serial symbol pass: ONE lane visits the non-Z tokens of every stretch in order (zero bits are skipped by count) and
//                      leaves each stretch its incoming (lastOccurred, second, third).  The format's second serial dependence.
//   k_sh_expand_blocks a lane per 16 output bytes: searches its record, writes the FILL and raw COPY bytes that fall into its 16 (16-byte accesses
//                      inside a record, bytes at its ends)
//   k_sh_expand_sym    a lane per stretch record: decodes its tokens from the incoming state.
#pragma once

#include "hsrle_common.hip.h"

namespace hsrle {

constexpr uint32_t kShDone = 0u, kShMalformed = 1u, kShCapacity = 2u;   // == HSRLE_RLE8_SH_* (include/hsrle.h)
constexpr uint32_t kShWinMax = 1024u, kShWinMin = 64u;
constexpr uint32_t kShFill = 0u, kShCopy = 1u, kShSym = 2u, kShSymEnc = 3u;   // record kinds
constexpr uint32_t kShMinStream = 13u;   // header, the terminator's u32, one bit byte

struct ShDecArgs
{
  const uint8_t *stream;
  uint8_t *out;
  uint4 *rec;            // x = output offset, y = body offset, z = bit offset (low word), w = kind | R << 8 | bit offset (high) << 16; [n] = the end
  uint2 *st;             // per record: x = lastOccurred | second << 8 | third << 16 in front of it ([n]: behind the last); y and, until the scan, x: the summary
  uint32_t *ctrl;        // [0] status, [1] records, [2] 1: the serial symbol pass runs (forced, or a proof failed), [3] stretches whose proof failed
  uint32_t *status;
  uint32_t streamCap, size, maxRec, cap, win, force;
};

// a value every lane holds alike, moved to the scalar side: what follows from it is scalar arithmetic and scalar branches
__device__ __forceinline__ uint32_t sh_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t sh_uniform64(uint64_t v) { return (uint64_t)sh_uniform((uint32_t)v) | (uint64_t)sh_uniform((uint32_t)(v >> 32)) << 32; }

// 16 bytes of the stream at `at`, zeros from `S` on
__device__ __forceinline__ u32x4 sh_ld_stream(const uint8_t *stream, uint64_t at, uint32_t S)
{
  u32x4 v = { 0u, 0u, 0u, 0u };
  if (at + 16u <= S) return ld128(stream + at);
  for (uint32_t k = 0; k < 16u && at + k < S; k++) v[k >> 2] |= (uint32_t)stream[at + k] << (8u * (k & 3u));
  return v;
}
// 16 bytes of the REVERSED stream (byte r of it is stream[S - 1 - r]) at `r0`, zeros from `S` on
__device__ __forceinline__ u32x4 sh_ld_reversed(const uint8_t *stream, uint64_t r0, uint32_t S)
{
  u32x4 v = { 0u, 0u, 0u, 0u };
  if (r0 + 16u <= S)
  {
    const u32x4 g = ld128(stream + (S - 16u - (uint32_t)r0));
    v[0] = __builtin_bswap32(g[3]); v[1] = __builtin_bswap32(g[2]); v[2] = __builtin_bswap32(g[1]); v[3] = __builtin_bswap32(g[0]);
    return v;
  }
  for (uint32_t k = 0; k < 16u && r0 + k < S; k++) v[k >> 2] |= (uint32_t)stream[S - 1u - (uint32_t)(r0 + k)] << (8u * (k & 3u));
  return v;
}
// 64 bits of the bit stream from bit `bit` on, straight from memory; zeros in front of the stream's first byte
__device__ __forceinline__ uint64_t sh_bits64(const uint8_t *stream, uint32_t S, uint64_t bit)
{
  const int64_t e = (int64_t)S - 1 - (int64_t)(bit >> 3);   // the byte that holds `bit`
  uint64_t lo = 0u, nxt = 0u;
  if (e >= 8)
  {
    lo = __builtin_bswap64(ld64(stream + (e - 7)));
    nxt = stream[e - 8];
  }
  else
    for (int64_t k = 0; k < 8 && e - k >= 0; k++) lo |= (uint64_t)stream[e - k] << (8 * k);
  const uint32_t s = (uint32_t)bit & 7u;
  return s ? (lo >> s) | (nxt << (64u - s)) : lo;
}

// The passes are __device__ functions of one argument block (and, where a lane has an index of its own, that index), so that the kernels of ONE
// stream below and the kernels of the blocked form (hsrle_rle8shb.hip.h: a workgroup that finds its own block) run the same code.
__device__ __forceinline__ void d_sh_walk(const ShDecArgs &a)
{
  __shared__ __attribute__((aligned(16))) uint64_t sBits[kShWinMax / 8u + 2u];
  __shared__ __attribute__((aligned(16))) uint8_t sBody[kShWinMax];
  const uint32_t lane = threadIdx.x, win = a.win, size = a.size;
  uint32_t status = kShDone, S = 0u;
  if (a.streamCap < kShMinStream) status = kShMalformed;
  else
  {
    S = sh_uniform(ld32(a.stream + 4));
    if (sh_uniform(ld32(a.stream)) != size || S > a.streamCap || S < kShMinStream) status = kShMalformed;
  }
  uint64_t bit = 0u, body = 8u, bitBase = 0u, bodyBase = 0u;
  uint32_t out = 0u, n = 0u, R = 0x7Fu, openCount = 0u;
  bool haveBits = false, haveBody = false, open = false, done = false;
  // 64 bits of the bit stream at `bit`, through the window of the reversed stream
  auto bits = [&]() -> uint64_t {
    const uint64_t rb = bit >> 3;
    if (!(haveBits && rb >= bitBase && rb + 16u <= bitBase + win))
    {
      __syncthreads();
      bitBase = rb;
      if (lane * 16u < win) lds_st128((uint8_t *)sBits + lane * 16u, sh_ld_reversed(a.stream, bitBase + lane * 16u, S));
      haveBits = true;
      __syncthreads();
    }
    const uint32_t k = (uint32_t)(rb - bitBase), s = (k & 7u) * 8u + ((uint32_t)bit & 7u);
    const uint64_t lo = sh_uniform64(sBits[k >> 3]), hi = sh_uniform64(sBits[(k >> 3) + 1u]);
    return s ? (lo >> s) | (hi << (64u - s)) : lo;
  };
  // after this call the body window holds [body, body + 8)
  auto need_body = [&]() {
    if (haveBody && body >= bodyBase && body + 8u <= bodyBase + win) return;
    __syncthreads();
    bodyBase = body;
    if (lane * 16u < win) lds_st128(sBody + lane * 16u, sh_ld_stream(a.stream, bodyBase + lane * 16u, S));
    haveBody = true;
    __syncthreads();
  };
  auto body8 = [&](uint32_t k) -> uint32_t { return sh_uniform(sBody[(uint32_t)(body - bodyBase) + k]); };
  auto body32 = [&]() -> uint32_t { return body8(0) | body8(1) << 8 | body8(2) << 16 | body8(3) << 24; };
  // the body cursor and the consumed bits have not met
  auto apart = [&]() -> bool { return body + ((bit + 7u) >> 3) <= S; };
  auto record = [&](uint32_t kind, uint64_t bodyOff) {
    if (lane == 0u) a.rec[n] = make_uint4(out, (uint32_t)bodyOff, (uint32_t)bit, kind | R << 8 | (uint32_t)(bit >> 32) << 16);
    n++;
  };
  while (status == kShDone && !done)
  {
    const uint64_t w = bits();
    if ((w & 0xFu) != 0xFu)
    {
      // a stretch of symbol tokens: up to the first 1-run of length >= 4 that shows whole in this word, else up to the word's last zero bit
      const uint64_t m4 = w & (w >> 1) & (w >> 2) & (w >> 3) & 0x1FFFFFFFFFFFFFFFull;
      const uint32_t p = m4 ? (uint32_t)__builtin_ctzll(m4) : 64u - (uint32_t)__builtin_clzll(~w);
      const uint64_t mask = p == 64u ? ~0ull : (1ull << p) - 1ull;
      const uint32_t sym = p - (uint32_t)__popcll(w & mask), lit = (uint32_t)__popcll(w & ~(w << 1) & ~(w >> 1) & mask);
      if (sym > size - out || n >= a.maxRec) { status = kShMalformed; break; }
      if (!open || openCount + sym > a.cap)
      {
        record(kShSym, body);
        open = true;
        openCount = 0u;
      }
      openCount += sym;
      bit += p;
      body += lit;
      out += sym;
      if (!apart()) status = kShMalformed;
      continue;
    }
    open = false;
    need_body();
    uint64_t cnt;
    if (!(w & 0x10u))
    {
      bit += 5u;
      cnt = body8(0) + 14u;
      body += 1u;
      if (cnt > size - out || n >= a.maxRec) { status = kShMalformed; break; }
      record(kShFill, 0u);
    }
    else
    {
      const uint32_t type = (uint32_t)(w >> 5) & 3u;
      bit += 7u;
      if (type == 0u || type == 1u)
      {
        if (type == 0u) { cnt = body8(0) + 7u; body += 1u; }
        else
        {
          cnt = body32();
          body += 4u;
          if (cnt == 0u)
          {
            if (!apart() || out != size) status = kShMalformed;
            done = true;
            break;
          }
          cnt += 7u;
        }
        if (cnt > size - out || n >= a.maxRec) { status = kShMalformed; break; }
        record(kShCopy, body);
        body += cnt;
      }
      else if (type == 2u)
      {
        cnt = (uint32_t)(body32() + 14u);
        R = body8(4);
        body += 5u;
        if (cnt > size - out || n >= a.maxRec || out == size) { status = kShMalformed; break; }   // (nothing but the terminator behind the last byte)
        if (cnt != 0u) record(kShFill, 0u);
      }
      else
      {
        cnt = body8(0) + 161u;
        body += 1u;
        if (cnt > size - out || n >= a.maxRec) { status = kShMalformed; break; }
        record(kShSymEnc, body);
        uint32_t left = (uint32_t)cnt;
        while (left != 0u && apart())
        {
          const uint64_t e = bits();
          uint32_t used = 0u;
          while (left != 0u && used <= 61u)
          {
            const uint32_t v = (uint32_t)(e >> used);
            if (!(v & 1u)) used += 1u;
            else if (!(v & 2u)) { used += 2u; body += 1u; }
            else used += 3u;
            left--;
          }
          bit += used;
        }
      }
    }
    out += (uint32_t)cnt;
    if (!apart()) status = kShMalformed;
  }
  if (lane == 0u)
  {
    if (status == kShDone) a.rec[n] = make_uint4(size, 0u, 0u, 0u);
    a.ctrl[0] = status;
    a.ctrl[1] = n;
    *a.status = status;
  }
}
template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_sh_walk(ShDecArgs a) { d_sh_walk(a); }

// Summary of a stretch, from its own tokens alone (a lane per stretch record): kind and value of its first and last token that is not Z
// (0 none, 1 L, 2 S, 3 T) and its SURE promotions -- a literal equal to the literal right in front of it -- of which the last two matter.
// x = first kind | last kind << 2 | promotions (0, 1, 2 = two and more) << 4 | first value << 8 | last value << 16, y = last promoted | the one before << 8.
// Left open: whether the FIRST token promotes (the scan knows the token in front of it) and whether a literal behind S / T promotes: THE GUESS is
// that it never does (no stream of the encoder has one: it tests second and third before it writes a literal).
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_sh_summary(ShDecArgs a)
{
  if (a.ctrl[0] != kShDone) return;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= a.ctrl[1]) return;
  const uint4 q = a.rec[i];
  const uint32_t kind = q.w & 3u;
  if (kind < kShSym) return;
  const uint32_t S = ld32(a.stream + 4), tBits = kind == kShSymEnc ? 3u : 4u;
  uint32_t cnt = a.rec[i + 1u].x - q.x, body = q.y;
  uint64_t bit = (uint64_t)q.z | (uint64_t)(q.w >> 16) << 32;
  uint32_t firstKind = 0u, firstVal = 0u, prevKind = 0u, prevVal = 0u, k = 0u, pLast = 0u, pPrev = 0u;
  while (cnt != 0u)
  {
    const uint64_t w = sh_bits64(a.stream, S, bit);
    uint32_t used = 0u;
    while (cnt != 0u && used <= 60u)
    {
      const uint64_t v = w >> used;
      if (!(v & 1u))
      {
        const uint32_t z = umin(umin(v ? (uint32_t)__builtin_ctzll(v) : 64u, 64u - used), cnt);
        used += z;
        cnt -= z;
        continue;
      }
      uint32_t tk, val = 0u;
      if (!(v & 2u)) { tk = 1u; val = a.stream[body++]; used += 2u; }
      else if (!(v & 4u)) { tk = 2u; used += 3u; }
      else { tk = 3u; used += tBits; }
      if (firstKind == 0u) { firstKind = tk; firstVal = val; }
      else if (tk == 1u && prevKind == 1u && val == prevVal) { pPrev = pLast; pLast = val; k = umin(k + 1u, 2u); }
      prevKind = tk;
      prevVal = val;
      cnt--;
    }
    bit += used;
  }
  a.st[i] = make_uint2(firstKind | prevKind << 2 | k << 4 | firstVal << 8 | prevVal << 16, pLast | pPrev << 8);
}

// A summary in its fields; a run of records has a summary of the same form, and putting two runs together is associative.
struct ShSum
{
  uint32_t fk, lk, k, fv, lv, p1, p0;   // first / last kind, promotions (2 = two and more), first / last value, last promoted, the one before
};
__device__ __forceinline__ ShSum sh_sum_unpack(uint2 s)
{
  ShSum r;
  r.fk = s.x & 3u; r.lk = (s.x >> 2) & 3u; r.k = (s.x >> 4) & 3u; r.fv = (s.x >> 8) & 0xFFu; r.lv = (s.x >> 16) & 0xFFu; r.p1 = s.y & 0xFFu; r.p0 = (s.y >> 8) & 0xFFu;
  return r;
}
__device__ __forceinline__ uint2 sh_sum_pack(const ShSum &r) { return make_uint2(r.fk | r.lk << 2 | r.k << 4 | r.fv << 8 | r.lv << 16, r.p1 | r.p0 << 8); }
__device__ __forceinline__ void sh_sum_push(ShSum &r, uint32_t v) { r.p0 = r.p1; r.p1 = v; r.k = umin(r.k + 1u, 2u); }
// A, then B.  Between them: B's first token promotes if it is a literal equal to the literal A ends in.
__device__ __forceinline__ ShSum sh_sum_join(const ShSum &A, const ShSum &B)
{
  if (B.fk == 0u) return A;
  if (A.fk == 0u) return B;
  ShSum r = A;
  r.lk = B.lk;
  r.lv = B.lv;
  if (A.lk == 1u && B.fk == 1u && A.lv == B.fv) sh_sum_push(r, B.fv);
  if (B.k == 1u) sh_sum_push(r, B.p1);
  else if (B.k == 2u) { r.p0 = B.p0; r.p1 = B.p1; r.k = 2u; }
  return r;
}
// The symbol state and the token in front (kind, value) behind a run of records with summary X
struct ShState
{
  uint32_t last, sec, third, curKind, curVal;
};
__device__ __forceinline__ void sh_state_apply(ShState &t, const ShSum &X)
{
  if (X.fk == 0u) return;
  if (X.fk == 1u && t.curKind == 1u && X.fv == t.curVal) { t.third = t.sec; t.sec = X.fv; }
  if (X.k == 1u) { t.third = t.sec; t.sec = X.p1; }
  else if (X.k == 2u) { t.third = X.p0; t.sec = X.p1; }
  t.last = X.lk == 1u ? X.lv : (X.lk == 2u ? t.sec : t.third);   // (nothing promotes behind the last token: S / T read the lists as they end)
  t.curKind = X.lk;
  t.curVal = X.lv;
}

// The scan over the summaries under the guess, a step per RECORD (not per token): one workgroup, a run of records per thread -- the run's
// summary, then thread 0 over the 1 024 runs (the one serial part: 1 024 steps), then every thread again through its run, leaving every record
// the state in front of it.
constexpr uint32_t kShScanThreads = 1024u;
template <int UNUSED = 0>
__global__ __launch_bounds__(1024) void k_sh_scan(ShDecArgs a)
{
  __shared__ uint2 sSum[kShScanThreads];
  __shared__ uint2 sIn[kShScanThreads];   // x = state, y = kind | value << 8 of the token in front
  const uint32_t t = threadIdx.x;
  if (t == 0u)
  {
    a.ctrl[2] = a.force ? 1u : 0u;
    a.ctrl[3] = 0u;
  }
  if (a.ctrl[0] != kShDone || a.force) return;
  const uint32_t n = a.ctrl[1], per = (n + kShScanThreads - 1u) / kShScanThreads;
  const uint32_t lo = umin(t * per, n), hi = umin(lo + per, n);
  ShSum acc = sh_sum_unpack(make_uint2(0u, 0u));
  for (uint32_t i = lo; i < hi; i++)
    if ((a.rec[i].w & 3u) >= kShSym) acc = sh_sum_join(acc, sh_sum_unpack(a.st[i]));
  sSum[t] = sh_sum_pack(acc);
  __syncthreads();
  if (t == 0u)
  {
    ShState s = { 0x80u, 0x80u, 0x7Eu, 1u, 0x80u };   // (the start value of lastOccurred acts as a literal in front)
    for (uint32_t j = 0; j < kShScanThreads; j++)
    {
      sIn[j] = make_uint2(s.last | s.sec << 8 | s.third << 16, s.curKind | s.curVal << 8);
      sh_state_apply(s, sh_sum_unpack(sSum[j]));
    }
    a.st[n].x = s.last | s.sec << 8 | s.third << 16;
  }
  __syncthreads();
  const uint2 in = sIn[t];
  ShState s = { in.x & 0xFFu, (in.x >> 8) & 0xFFu, (in.x >> 16) & 0xFFu, in.y & 0xFFu, (in.y >> 8) & 0xFFu };
  for (uint32_t i = lo; i < hi; i++)
  {
    const uint32_t state = s.last | s.sec << 8 | s.third << 16;
    if ((a.rec[i].w & 3u) < kShSym) { a.st[i].x = state; continue; }
    const uint2 q = a.st[i];
    a.st[i].x = state;
    sh_state_apply(s, sh_sum_unpack(q));
  }
}

// THE FALLBACK, and the simplest correct decoder of the symbol state: one lane, every stretch in order.  Zero bits are skipped by count, so the
// cost is per L / S / T token.  It runs when a proof of k_sh_expand_sym<0> failed or when hsrle_rle8_sh_tuning forces it.
__device__ __forceinline__ void d_sh_state(const ShDecArgs &a)
{
  if (threadIdx.x != 0u || a.ctrl[0] != kShDone || a.ctrl[2] == 0u) return;
  const uint32_t n = a.ctrl[1], S = ld32(a.stream + 4);
  uint32_t last = 0x80u, sec = 0x80u, third = 0x7Eu;
  for (uint32_t i = 0; i < n; i++)
  {
    const uint4 q = a.rec[i];
    const uint32_t kind = q.w & 3u;
    if (kind < kShSym) continue;
    a.st[i].x = last | sec << 8 | third << 16;
    const uint32_t tBits = kind == kShSymEnc ? 3u : 4u;
    uint32_t cnt = a.rec[i + 1u].x - q.x, body = q.y, have = 0u;
    uint64_t bit = (uint64_t)q.z | (uint64_t)(q.w >> 16) << 32, lits = 0u;
    while (cnt != 0u)
    {
      const uint64_t w = sh_bits64(a.stream, S, bit);
      uint32_t used = 0u;
      while (cnt != 0u && used <= 60u)
      {
        const uint64_t v = w >> used;
        if (!(v & 1u))
        {
          const uint32_t z = umin(umin(v ? (uint32_t)__builtin_ctzll(v) : 64u, 64u - used), cnt);
          used += z;
          cnt -= z;
          continue;
        }
        if (!(v & 2u))
        {
          if (have == 0u)   // the next 8 body bytes (the walk has seen that every literal lies inside the stream)
          {
            lits = 0u;
            if (body + 8u <= S) lits = ld64(a.stream + body);
            else for (uint32_t k = 0; body + k < S; k++) lits |= (uint64_t)a.stream[body + k] << (8u * k);
            have = 8u;
          }
          const uint32_t sym = (uint32_t)lits & 0xFFu;
          lits >>= 8;
          have--;
          body++;
          if (sym == last) { third = sec; sec = sym; }
          last = sym;
          used += 2u;
        }
        else if (!(v & 4u)) { last = sec; used += 3u; }
        else { last = third; used += tBits; }
        cnt--;
      }
      bit += used;
    }
  }
}
template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_sh_state(ShDecArgs a) { d_sh_state(a); }

// `lane`: the 16 output bytes [16 lane, 16 lane + 16)
__device__ __forceinline__ void d_sh_expand_blocks(const ShDecArgs &a, uint64_t lane)
{
  if (a.ctrl[0] != kShDone) return;
  const uint64_t c64 = lane * 16u;
  if (c64 >= a.size) return;
  const uint32_t c0 = (uint32_t)c64, c1 = umin(a.size - c0, 16u) + c0, n = a.ctrl[1];
  uint32_t lo = 0u, hi = n;   // (record 0 starts at output offset 0, the offsets rise strictly)
  while (hi - lo > 1u)
  {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (a.rec[mid].x <= c0) lo = mid; else hi = mid;
  }
  for (uint32_t i = lo; i < n; i++)
  {
    const uint4 q = a.rec[i];
    if (q.x >= c1) break;
    const uint32_t kind = q.w & 3u;
    if (kind >= kShSym) continue;
    const uint32_t s = q.x > c0 ? q.x : c0, e = umin(a.rec[i + 1u].x, c1);
    if (kind == kShFill)
    {
      const uint32_t r = (q.w >> 8) & 0xFFu, r4 = r * 0x01010101u;
      const u32x4 v = { r4, r4, r4, r4 };
      if (e - s == 16u) st128(a.out + s, v);
      else for (uint32_t k = s; k < e; k++) a.out[k] = (uint8_t)r;
    }
    else
    {
      const uint8_t *src = a.stream + q.y + (s - q.x);
      if (e - s == 16u) st128(a.out + s, ld128(src));
      else for (uint32_t k = 0; k < e - s; k++) a.out[s + k] = src[k];
    }
  }
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_sh_expand_blocks(ShDecArgs a) { d_sh_expand_blocks(a, (uint64_t)blockIdx.x * 256u + threadIdx.x); }

// PASS 0: from the scan's states; every lane PROVES the guess for its stretch: the state it ends in must be the state the scan gave the next
// record.  If that holds for every stretch, every state of the scan is the true one (by induction from the first); if not, ctrl[2] gates the
// fallback.  PASS 1: again, from the serial pass's states, only when ctrl[2] is set.
template <int PASS>
__device__ __forceinline__ void d_sh_expand_sym(const ShDecArgs &a, uint32_t i)
{
  if (a.ctrl[0] != kShDone) return;
  if (PASS == 0 ? a.force != 0u : a.ctrl[2] == 0u) return;
  if (i >= a.ctrl[1]) return;
  const uint4 q = a.rec[i];
  const uint32_t kind = q.w & 3u;
  if (kind < kShSym) return;
  const uint32_t S = ld32(a.stream + 4), R = (q.w >> 8) & 0xFFu, st = a.st[i].x, tBits = kind == kShSymEnc ? 3u : 4u;
  uint32_t last = st & 0xFFu, sec = (st >> 8) & 0xFFu, third = (st >> 16) & 0xFFu;
  uint32_t o = q.x, cnt = a.rec[i + 1u].x - q.x, body = q.y;
  uint64_t bit = (uint64_t)q.z | (uint64_t)(q.w >> 16) << 32;
  while (cnt != 0u)
  {
    const uint64_t w = sh_bits64(a.stream, S, bit);
    uint32_t used = 0u;
    while (cnt != 0u && used <= 60u)
    {
      const uint32_t v = (uint32_t)(w >> used);
      uint32_t sym;
      if (!(v & 1u)) { sym = R; used += 1u; }
      else if (!(v & 2u))
      {
        sym = a.stream[body++];
        if (sym == last) { third = sec; sec = sym; }
        last = sym;
        used += 2u;
      }
      else if (!(v & 4u)) { sym = sec; last = sym; used += 3u; }
      else { sym = third; last = sym; used += tBits; }
      a.out[o++] = (uint8_t)sym;
      cnt--;
    }
    bit += used;
  }
  if (PASS == 0 && (last | sec << 8 | third << 16) != a.st[i + 1u].x)
  {
    atomicOr(&a.ctrl[2], 1u);
    atomicAdd(&a.ctrl[3], 1u);
  }
}
template <int PASS>
__global__ __launch_bounds__(256) void k_sh_expand_sym(ShDecArgs a) { d_sh_expand_sym<PASS>(a, blockIdx.x * 256u + threadIdx.x); }

// ------------------------------------------------------------------------------------------------------------------
// encode
//
// The reference's byte loop (rle_sh.c:300-505) restated as a loop over MAXIMAL RUNS of equal bytes (tools/rle8_sh_model.py): what is emitted -- FILL,
// change of R, raw COPY, plain or encoded symbol stretch -- depends on R, the run lengths, three counters and one flag, never on second / third.
//   k_she_decide   ONE wave: 1 KiB windows, a lane per 16 bytes marks the bytes that differ from their predecessor; the wave then consumes RUNS,
//                  not bytes, and leaves one item per decision (input offset, count, kind, R)
//   k_she_code     ONE lane follows second / third / lastOccurred through the bytes of the symbol stretches (raw COPY and FILL bytes are not
//                  touched; eight bytes of R at once), cuts encoded copies into their blocks of 416 and gives every emission record its body
//                  offset, bit offset and incoming state; the stream size, the size word and the status come from here
//   k_she_zero     zeroes the words of the workspace's bit buffer that this stream fills (the token bits are ORed into it)
//   k_she_emit     a lane per emission record: token bits into the bit buffer, counts / new R / literals into the body
//   k_she_raw      a lane per 16 input bytes: the bodies of the raw COPYs
//   k_she_place    the bit buffer, byte-reversed, behind the body; the header
constexpr uint32_t kSeRaw = 0u, kSeSym = 1u, kSeSpan = 2u, kSeFill = 3u, kSeChange = 4u, kSeChunk = 5u, kSeEnd = 6u;

struct ShEncArgs
{
  const uint8_t *in;
  uint8_t *out;
  uint4 *items;          // x = input offset, y = count, z = kind | R << 8 (CHANGE: the new R)
  uint4 *er;             // two per emission record: (input offset, count, kind | R << 8, lastOccurred | second << 8 | third << 16), (body offset, bit offset lo, hi, 0)
  uint32_t *bits;        // bit k of the bit stream is bit k % 32 of word k / 32
  uint32_t *ctrl;        // [0] 1: does not fit, [1] items, [2] emission records, [3] stream size, [4] bytes of the bit stream
  uint32_t *outSize, *status;
  uint32_t size, maxItems, maxEr, bitWords, outCap;
};

__device__ __forceinline__ void d_she_zero(const ShEncArgs &a, uint32_t i)
{
  if (a.ctrl[0] == 0u && (uint64_t)i * 4u < a.ctrl[4]) a.bits[i] = 0u;   // (only the words the bit stream will fill: k_she_code has counted them)
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_she_zero(ShEncArgs a) { d_she_zero(a, blockIdx.x * 256u + threadIdx.x); }

__device__ __forceinline__ void d_she_decide(const ShEncArgs &a)
{
  __shared__ __attribute__((aligned(16))) uint8_t sWin[1024];
  __shared__ __attribute__((aligned(16))) uint64_t sMask[16], sIsR[16];
  const uint32_t lane = threadIdx.x, n = a.size;
  uint32_t R = 0x7Fu, block = 0u, count = 0u, rIn = 0u, pend = 0u, change = 0u, prev = 0u, nItems = 0u;
  bool inCopy = false, overflow = false;
  auto item = [&](uint32_t kind, uint32_t pos, uint32_t cnt, uint32_t sym) {
    if (cnt == 0u) return;
    if (nItems >= a.maxItems) { overflow = true; return; }
    if (lane == 0u) a.items[nItems] = make_uint4(pos, cnt, kind | sym << 8, 0u);
    nItems++;
  };
  auto copy = [&](uint32_t pos, uint32_t cnt) { item(cnt >= 7u ? kSeRaw : kSeSym, pos, cnt, R); };
  auto blk = [&](uint32_t pos, uint32_t cnt, uint32_t r) {   // the 7 : 2 rule
    if ((uint64_t)r * 7u > (uint64_t)(cnt - r) * 2u) item(kSeSpan, pos, cnt, R); else copy(pos, cnt);
  };
  auto fill = [&](uint32_t pos, uint32_t cnt) { item(cnt >= 14u ? kSeFill : kSeSym, pos, cnt, R); };
  auto run = [&](uint32_t pos, uint32_t v, uint32_t len) {
    if (v == R && change >= 10u)
    {
      copy(block, count - change);
      R = prev;
      item(kSeChange, pos - change, change, R);
      block = pos; count = len; rIn = 0u; pend = 0u; change = len;
    }
    else if (v == R)
    {
      rIn += len;
      pend = len;
      change = 0u;
      if (len > 14u)
      {
        blk(block, count, rIn - len);
        block = pos; count = 0u; rIn = 0u; inCopy = false;
      }
    }
    else
    {
      if (pend != 0u && inCopy) { count += pend; pend = 0u; }
      if (change >= 10u)
      {
        blk(block, count - change, rIn);
        R = prev;
        item(kSeChange, pos - change, change, R);
        block = pos; count = 0u; rIn = 0u;
      }
      if (!inCopy)
      {
        fill(pos - pend, pend);
        block = pos; count = 0u; rIn = 0u; pend = 0u; inCopy = true;
      }
      count += len;
      change = len;
    }
    prev = v;
  };
  uint32_t runStart = 0u, runSym = 0u, carry = 0u;
  for (uint32_t base = 0u; base < n; base += 1024u)
  {
    __syncthreads();
    const uint32_t at = base + lane * 16u;
    u32x4 v = { 0u, 0u, 0u, 0u };
    if (at + 16u <= n) v = ld128(a.in + at);
    else for (uint32_t k = 0; k < 16u && at + k < n; k++) v[k >> 2] |= (uint32_t)a.in[at + k] << (8u * (k & 3u));
    lds_st128(sWin + lane * 16u, v);
    uint32_t before = __shfl_up(v[3], 1, 64);
    if (lane == 0u) before = carry;
    carry = __shfl(v[3], 63, 64);
    const uint32_t R0 = R, r4 = R * 0x01010101u;   // (the bytes equal to the R of the window's start; R changes at events only)
    uint32_t m = 0u, isR = 0u;
#pragma unroll
    for (int d = 0; d < 4; d++)
    {
      const uint32_t t = v[d] ^ (v[d] << 8 | before >> 24), u = v[d] ^ r4;
      const uint32_t nz = (((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u, nr = (((u & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | u) & 0x80808080u;
      m |= ((((nz >> 7) * 0x01020408u) >> 24) & 0xFu) << (4 * d);
      isR |= (((((nr ^ 0x80808080u) >> 7) * 0x01020408u) >> 24) & 0xFu) << (4 * d);
      before = v[d];
    }
    if (at == 0u) m |= 1u;
    ((uint16_t *)sMask)[lane] = (uint16_t)m;
    ((uint16_t *)sIsR)[lane] = (uint16_t)isR;
    __syncthreads();
    for (uint32_t w = 0; w < 16u; w++)
    {
      uint64_t mm = sh_uniform64(sMask[w]);
      if (base + w * 64u + 64u > n) mm &= (1ull << ((n - base) & 63u)) - 1ull;   // (a last, partial word: nothing behind the input's end)
      // Runs that begin AND end in this word, none of them of R, none of 10 bytes: they only add to the open block.  Such a stretch is taken at
      // once as soon as the state is plain (a block is open, nothing pends, the run before was short).
      const uint64_t z = ~mm, z2 = z & (z >> 1), z4 = z2 & (z2 >> 2), z8 = z4 & (z4 >> 4), z9 = z8 & (z >> 8);
      const uint32_t lastBit = mm ? 63u - (uint32_t)__builtin_clzll(mm) : 0u;
      const uint64_t r64 = sh_uniform64(sIsR[w]);
      while (mm)
      {
        const uint32_t b = (uint32_t)__builtin_ctzll(mm), pos = base + w * 64u + b;
        mm &= mm - 1ull;
        if (pos != 0u) run(runStart, runSym, pos - runStart);
        runStart = pos;
        runSym = sh_uniform(sWin[pos - base]);
        // The shortcut.  For a run that is not of R, run() does nothing but `count += len; change = len; prev = v` once four things hold:
        //   inCopy       a block is open (else the run would first emit the pending FILL and open one)
        //   pend == 0    no run of R waits to be merged into the block
        //   change < 10  the run before it does not become the new R
        //   R == R0      sIsR was made for the R of the window's start: after a change of R inside the window it says nothing
        // and a run of under 10 bytes leaves them all true.  So the whole runs from here to the word's last start (`span`) are taken at once if
        // none of them holds a byte of R and none is 10 bytes long, i.e. no 9 non-starts in a row lie inside the span (bit lastBit is a start,
        // so nine zeros that begin inside the span end inside it).
        if (mm != 0u && R == R0 && inCopy && pend == 0u && change < 10u)
        {
          const uint64_t span = ((1ull << lastBit) - 1ull) & ~((1ull << b) - 1ull);   // bits b .. lastBit - 1
          if ((r64 & span) == 0u && (z9 & span) == 0u)
          {
            const uint64_t inner = mm & ~(1ull << lastBit);
            const uint32_t lastRun = inner ? 63u - (uint32_t)__builtin_clzll(inner) : b;   // where the last whole run begins
            count += lastBit - b;
            change = lastBit - lastRun;
            prev = sh_uniform(sWin[w * 64u + lastRun]);
            runStart = base + w * 64u + lastBit;
            runSym = sh_uniform(sWin[w * 64u + lastBit]);
            mm = 0u;
          }
        }
      }
    }
  }
  run(runStart, runSym, n - runStart);
  if (inCopy) copy(block, count + pend); else fill(n - pend, pend);
  if (lane == 0u)
  {
    a.ctrl[0] = overflow ? 1u : 0u;
    a.ctrl[1] = nItems;
  }
}
template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_she_decide(ShEncArgs a) { d_she_decide(a); }

__device__ __forceinline__ void d_she_code(const ShEncArgs &a)
{
  if (threadIdx.x != 0u) return;
  const uint32_t n = a.size, nItems = a.ctrl[1];
  bool bad = a.ctrl[0] != 0u;
  uint32_t body = 8u, last = 0x80u, sec = 0x80u, third = 0x7Eu, ne = 0u;
  uint64_t bit = 0u;
  auto rec = [&](uint32_t pos, uint32_t cnt, uint32_t kind, uint32_t R) {
    if (ne >= a.maxEr) { bad = true; return; }
    a.er[2u * ne] = make_uint4(pos, cnt, kind | R << 8, last | sec << 8 | third << 16);
    a.er[2u * ne + 1u] = make_uint4(body, (uint32_t)bit, (uint32_t)(bit >> 32), 0u);
    ne++;
  };
  auto code = [&](uint32_t pos, uint32_t cnt, uint32_t R, uint32_t tBits) {
    const uint64_t r8 = R * 0x0101010101010101ull;
    while (cnt != 0u)
    {
      const uint32_t k = umin(cnt, 8u);
      uint64_t w = 0u;
      if (pos + 8u <= n) w = ld64(a.in + pos);
      else for (uint32_t j = 0; j < k; j++) w |= (uint64_t)a.in[pos + j] << (8u * j);
      if (k == 8u && w == r8) bit += 8u;
      else
        for (uint32_t j = 0; j < k; j++)
        {
          const uint32_t v = (uint32_t)(w >> (8u * j)) & 0xFFu;
          if (v == R) bit += 1u;
          else if (v == sec) { bit += 3u; last = v; }
          else if (v == third) { bit += tBits; last = v; }
          else
          {
            bit += 2u;
            body += 1u;
            if (v == last) { third = sec; sec = v; }
            last = v;
          }
        }
      pos += k;
      cnt -= k;
    }
  };
  for (uint32_t i = 0; i < nItems && !bad; i++)
  {
    const uint4 q = a.items[i];
    const uint32_t kind = q.z & 0xFFu, R = (q.z >> 8) & 0xFFu, cnt = q.y;
    if (kind == kSeRaw) { rec(q.x, cnt, kind, R); bit += 7u; body += (cnt > 262u ? 4u : 1u) + cnt; }
    else if (kind == kSeFill)
    {
      rec(q.x, cnt, kind, R);
      if (cnt > 269u) { bit += 7u; body += 5u; } else { bit += 5u; body += 1u; }
    }
    else if (kind == kSeChange) { rec(q.x, cnt, kind, R); bit += 7u; body += 5u; }
    else if (kind == kSeSym) { rec(q.x, cnt, kSeSym, R); code(q.x, cnt, R, 4u); }
    else
    {
      uint32_t pos = q.x, rem = cnt;
      while (rem > 161u && !bad)
      {
        const uint32_t c = umin(rem, 416u);
        rec(pos, c, kSeChunk, R);
        bit += 7u;
        body += 1u;
        code(pos, c, R, 3u);
        pos += c;
        rem -= c;
      }
      if (rem != 0u) { rec(pos, rem, kSeSym, R); code(pos, rem, R, 4u); }
    }
  }
  rec(n, 0u, kSeEnd, 0u);
  bit += 7u;
  body += 4u;
  const uint64_t bitBytes = (bit + 7u) >> 3, total = body + bitBytes;
  const bool fits = !bad && total <= a.outCap && bitBytes <= (uint64_t)a.bitWords * 4u;
  a.ctrl[0] = fits ? 0u : 1u;
  a.ctrl[2] = ne;
  a.ctrl[3] = (uint32_t)total;
  a.ctrl[4] = (uint32_t)bitBytes;
  *a.outSize = fits ? (uint32_t)total : 0u;
  *a.status = fits ? kShDone : kShCapacity;
}
template <int UNUSED = 0>
__global__ __launch_bounds__(64) void k_she_code(ShEncArgs a) { d_she_code(a); }

__device__ __forceinline__ void d_she_emit(const ShEncArgs &a, uint32_t e)
{
  if (a.ctrl[0] != 0u) return;
  if (e >= a.ctrl[2]) return;
  const uint4 q = a.er[2u * e], o = a.er[2u * e + 1u];
  const uint32_t kind = q.z & 0xFFu, R = (q.z >> 8) & 0xFFu, cnt = q.y;
  uint32_t body = o.x;
  const uint64_t bit = (uint64_t)o.y | (uint64_t)o.z << 32;
  uint32_t word = (uint32_t)(bit >> 5), have = (uint32_t)bit & 31u;
  uint64_t acc = 0u;
  auto put = [&](uint32_t v, uint32_t c) {
    acc |= (uint64_t)v << have;
    have += c;
    if (have >= 32u)
    {
      atomicOr(&a.bits[word], (uint32_t)acc);
      acc >>= 32;
      have -= 32u;
      word++;
    }
  };
  if (kind == kSeRaw)
  {
    if (cnt > 262u) { put(0x3Fu, 7u); st32(a.out + body, cnt - 7u); }
    else { put(0x1Fu, 7u); a.out[body] = (uint8_t)(cnt - 7u); }
  }
  else if (kind == kSeFill)
  {
    if (cnt > 269u) { put(0x5Fu, 7u); st32(a.out + body, cnt - 14u); a.out[body + 4u] = (uint8_t)R; }
    else { put(0x0Fu, 5u); a.out[body] = (uint8_t)(cnt - 14u); }
  }
  else if (kind == kSeChange) { put(0x5Fu, 7u); st32(a.out + body, cnt - 14u); a.out[body + 4u] = (uint8_t)R; }
  else if (kind == kSeEnd) { put(0x3Fu, 7u); st32(a.out + body, 0u); }
  else
  {
    uint32_t last = q.w & 0xFFu, sec = (q.w >> 8) & 0xFFu, third = (q.w >> 16) & 0xFFu;
    const bool enc = kind == kSeChunk;
    if (enc) { put(0x7Fu, 7u); a.out[body++] = (uint8_t)(cnt - 161u); }
    for (uint32_t k = 0; k < cnt; k++)
    {
      const uint32_t v = a.in[q.x + k];
      if (v == R) put(0u, 1u);
      else if (v == sec) { put(3u, 3u); last = v; }
      else if (v == third) { if (enc) put(7u, 3u); else put(7u, 4u); last = v; }
      else
      {
        put(1u, 2u);
        if (v == last) { third = sec; sec = v; }
        last = v;
        a.out[body++] = (uint8_t)v;
      }
    }
  }
  if (have != 0u) atomicOr(&a.bits[word], (uint32_t)acc);
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_she_emit(ShEncArgs a) { d_she_emit(a, blockIdx.x * 256u + threadIdx.x); }

// `lane`: the 16 input bytes [16 lane, 16 lane + 16)
__device__ __forceinline__ void d_she_raw(const ShEncArgs &a, uint64_t lane)
{
  if (a.ctrl[0] != 0u) return;
  const uint64_t c64 = lane * 16u;
  if (c64 >= a.size) return;
  const uint32_t c0 = (uint32_t)c64, c1 = umin(a.size - c0, 16u) + c0, ne = a.ctrl[2];
  uint32_t lo = 0u, hi = ne;   // (record 0 starts at input offset 0, the offsets rise strictly, the last record is the END at `size`)
  while (hi - lo > 1u)
  {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (a.er[2u * mid].x <= c0) lo = mid; else hi = mid;
  }
  for (uint32_t i = lo; i < ne; i++)
  {
    const uint4 q = a.er[2u * i];
    if (q.x >= c1) break;
    if ((q.z & 0xFFu) != kSeRaw) continue;
    const uint32_t s = q.x > c0 ? q.x : c0, e = umin(q.x + q.y, c1);
    uint8_t *dst = a.out + a.er[2u * i + 1u].x + (q.y > 262u ? 4u : 1u) + (s - q.x);
    if (e - s == 16u) st128(dst, ld128(a.in + s));
    else for (uint32_t k = 0; k < e - s; k++) dst[k] = a.in[s + k];
  }
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_she_raw(ShEncArgs a) { d_she_raw(a, (uint64_t)blockIdx.x * 256u + threadIdx.x); }

__device__ __forceinline__ void d_she_place(const ShEncArgs &a, uint32_t g)
{
  if (a.ctrl[0] != 0u) return;
  const uint32_t total = a.ctrl[3], bitBytes = a.ctrl[4];
  if (g == 0u) { st32(a.out, a.size); st32(a.out + 4, total); }
  if ((uint64_t)g * 4u >= bitBytes) return;
  const uint32_t w = a.bits[g];
  for (uint32_t j = 0; j < 4u && g * 4u + j < bitBytes; j++) a.out[total - 1u - (g * 4u + j)] = (uint8_t)(w >> (8u * j));
}
template <int UNUSED = 0>
__global__ __launch_bounds__(256) void k_she_place(ShEncArgs a) { d_she_place(a, blockIdx.x * 256u + threadIdx.x); }

}   // namespace hsrle
