// hsrle_capi_dropin.h -- part of hsrle_capi.hip: the host-pointer (rle.h drop-in) functions of all families, each on one Staging (hsrle_capi_host.h)
#pragma once
#include "hsrle_capi_mono_decode.h"
#include "hsrle_capi_mono_encode.h"
#include "hsrle_capi_low_entropy.h"

namespace hsrle {

static uint32_t mono_compress(int codec, const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize)
{
  // argument checks of the reference (rle8_extreme_cpu.h:88-89, rleX_extreme_cpu.h:49-50, rleX_Xsl.h:271-272)
  if (pIn == nullptr || inSize == 0 || pOut == nullptr || outSize < bounds32(inSize))
    return 0;
  if (inSize > (1u << 30)) // A.5 q8: sizes above 1 GiB cannot be bounded; treated as unsupported
    return 0;
  if (codec < 0 || codec >= kCodecCount || !device_ok())
    return 0;

  init_tables();
  if (!g_launch[codec].enc)
    return 0;

  Staging s;
  const uint32_t stride = (bounds32(inSize) + 15u) & ~15u;
  if (!s.reserve(inSize, stride))
    return 0;

  // many lanes where the codec allows it (cuts behind long runs, hsrle_mono_encode.hip.h); else -- and for inputs of one piece -- one lane
  if (g_launch[codec].menc)
  {
    const MonoEncPlan m = plan_mono_encode(inSize, codec);
    if (m.pieces >= 2u)
    {
      if (!s.reserve_ws(m.total, kMonoWs) || !s.up(pIn, inSize))
        return 0;
      uint32_t size = 0;
      const int rc = mono_encode_dev(codec, s.in, inSize, s.out, s.ws, m, &size, nullptr, nullptr);
      if (rc == HSRLE_OK)
        return (size != 0 && size <= outSize && s.down(pOut, s.out, size)) ? size : 0;
      if (rc != HSRLE_ERR_UNSUPPORTED)                                   // (UNSUPPORTED: the list guesses did not settle -- one lane, below)
        return 0;
    }
  }
  if (!s.up(pIn, inSize))
    return 0;
  EncodeArgs ea{ s.in, inSize, inSize, 1u, s.out, stride, s.status };
  if (g_launch[codec].enc(ea, nullptr) != hipSuccess)
    return 0;
  uint32_t size = 0;
  if (!s.words(&size, s.status, 1) || size == 0 || size > outSize || !s.down(pOut, s.out, size))
    return 0;
  return size;
}

static uint32_t mono_decompress(int codec, const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize)
{
  // argument + header checks of the reference (rle8_extreme_cpu.h:704-712, rleX_extreme_cpu.h:84-91, rleX_Xsl.h:1850-1858)
  if (pIn == nullptr || pOut == nullptr || inSize == 0 || outSize == 0)
    return 0;
  if (codec < 0 || codec >= kCodecCount || inSize < header_size(kCodecs[codec]))
    return 0;
  uint8_t h16[16] = { 0 };
  memcpy(h16, pIn, inSize < 16u ? inSize : 16u);
  MonoHeader mh;
  if (!mono_header(codec, h16, inSize, outSize, &mh) || !device_ok())
    return 0;

  const MonoPlan m = plan_mono(mh.codec, mh.U, mh.C, mh.p0);
  Staging s;
  if (!s.reserve(mh.C, mh.U) || !s.reserve_ws(m.total, kMonoWs) || !s.up(pIn, mh.C, 0, 128))
    return 0;
  if (mono_decode_dev(mh, s.in, s.out, s.ws, m, nullptr, nullptr) != HSRLE_OK || !s.down(pOut, s.out, mh.U))
    return 0;
  return mh.U;
}

static uint32_t rle8m_mono_compress(uint32_t sections, const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize)
{
  // argument checks of the reference (rle8_low_entropy_cpu.c:133-134)
  if (pIn == nullptr || inSize == 0 || pOut == nullptr || sections == 0 || outSize < rle8m_bounds(sections, inSize) || !device_ok())
    return 0;
  const Rle8mPlan p = plan_rle8m(inSize, sections);
  Staging s;
  if (!s.reserve(inSize, outSize) || !s.reserve_ws(p.total) || !s.up(pIn, inSize))
    return 0;
  if (rle8m_encode_async(s.in, inSize, sections, s.out, outSize, s.ws, s.wsSize, s.status, nullptr) != HSRLE_OK)
    return 0;
  uint32_t status = 1, size = 0;
  if (!s.words(&status, s.status, 1) || status != 0 || !s.words(&size, s.out, 1) || size == 0 || size > outSize || !s.down(pOut, s.out, size))
    return 0;
  return size;
}

static uint32_t rle8m_mono_decompress(const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize)
{
  // argument + header checks of the reference (rle8_ocl.c:267-283, rle8_low_entropy_cpu.c:195-211)
  if (pIn == nullptr || pOut == nullptr || inSize < 12 || outSize == 0)
    return 0;
  uint32_t expIn, expOut, sections;
  memcpy(&expIn, pIn, 4); memcpy(&expOut, pIn + 4, 4); memcpy(&sections, pIn + 8, 4);
  if (expOut > outSize || expIn > inSize || sections == 0 || expOut == 0 || !device_ok())
    return 0;

  Staging s;
  if (!s.reserve(expIn, expOut) || !s.up(pIn, expIn))
    return 0;
  if (rle8m_decode_async(s.in, expIn, expOut, sections, s.out, expOut, s.status, nullptr) != HSRLE_OK)
    return 0;
  uint32_t status = 1;
  if (!s.words(&status, s.status, 1) || status != 0 || !s.down(pOut, s.out, expOut))
    return 0;
  return expOut;
}

static uint32_t le_mono_compress(const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize, uint32_t maxLen, uint32_t onlyMax)
{
  // argument checks of the reference (rle8_low_entropy_cpu.c:13-14; the Short form checks against the same bound, rle8_low_entropy_short_cpu.c:23)
  if (pIn == nullptr || inSize == 0 || pOut == nullptr || outSize < le_bounds(inSize) || !device_ok())
    return 0;
  const LePlan p = plan_le(inSize, true);
  Staging s;
  if (!s.reserve(inSize, outSize) || !s.reserve_ws(p.total) || !s.up(pIn, inSize))
    return 0;
  if (le_encode_async(s.in, inSize, s.out, outSize, s.ws, s.wsSize, s.status, maxLen, onlyMax, nullptr) != HSRLE_OK)
    return 0;
  uint32_t status = 1, size = 0;
  if (!s.words(&status, s.status, 1) || status != 0 || !s.words(&size, s.out, 1) || size < 8u + 33u || size > outSize || !s.down(pOut, s.out, size))
    return 0;
  return size;
}

static uint32_t le_mono_decompress(const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize)
{
  // argument + header checks of the reference (rle8_low_entropy_cpu.c:98-107)
  if (pIn == nullptr || pOut == nullptr || inSize < 8u + 33u || outSize == 0 || !device_ok())
    return 0;
  uint32_t expIn, expOut;
  memcpy(&expIn, pIn, 4); memcpy(&expOut, pIn + 4, 4);
  if (expOut > outSize || expIn > inSize || expIn < 8u + 33u || expOut == 0 || expIn > 0xFFFFFF00u)
    return 0;
  uint32_t listed = pIn[8 + 32];
  if (listed == 0u) listed = 255u;
  const uint32_t dataStart = 8u + 33u + listed;
  if (dataStart > expIn)
    return 0;
  const uint64_t many = plan_le(expIn - dataStart, false).total, one = plan_le(expIn - dataStart, false, expIn + 128u).total;   // (either attempt of le_decode_attempts)
  Staging s;
  if (!s.reserve(expIn, expOut) || !s.reserve_ws(many > one ? many : one) || !s.up(pIn, expIn, 0, 128))
    return 0;
  if (le_decode_attempts(s.in, expIn, dataStart, expOut, s.out, expOut, s.ws, s.wsSize, s.status, nullptr) != HSRLE_OK || !s.down(pOut, s.out, expOut))
    return 0;
  return expOut;
}

// ---- the split-phase helpers (src/rle.h:67-96): statistics, header writer / reader and the stream bodies as separate calls, tables through host structs ----

// rle8_low_entropy_get_compress_info[_only_max_frequency] (rle8_low_entropy_cpu.c:254-439): the statistics and table kernels of le_encode_async, tables back to the host
static bool le_get_info(const uint8_t *pIn, uint32_t inSize, rle8_low_entropy_compress_info_t *info, uint32_t onlyMax)
{
  if (pIn == nullptr || inSize == 0 || info == nullptr || !device_ok())
    return false;
  const LePlan p = plan_le(inSize, false);
  Staging s;
  if (!s.reserve(inSize, 0) || !s.reserve_ws(p.total))
    return false;
  Rle8mTables *t = (Rle8mTables *)(s.ws + p.offTables);
  if (!s.up(pIn, inSize) || zero_async(t, sizeof(Rle8mTables), nullptr) != hipSuccess)
    return false;
  if (launch_le_stats(s.in, inSize, t, 255u, s.ws + p.offStats, nullptr) != hipSuccess)
    return false;
  hipLaunchKernelGGL(k_rle8m_info, dim3(1), dim3(256), 0, nullptr, t, 1u, s.ws + p.offTmpInfo, onlyMax);
  Rle8mTables ht;
  uint8_t used = 0;
  if (hipGetLastError() != hipSuccess || !s.down(&ht, t, sizeof(ht)) || !s.down(&used, s.ws + p.offTmpInfo + 12u + 32u, 1))
    return false;
  for (int i = 0; i < 256; i++) { info->rle[i] = ht.rle[i] != 0; info->symbolsByProb[i] = ht.order[i]; }
  info->symbolCount = used;                                              // (a uint8: 256 symbols in use -> 0, rle8_low_entropy_cpu.c:333)
  return true;
}

// rle8_low_entropy[_short]_compress_with_info (rle8_low_entropy_cpu.c:474-543, rle8_low_entropy_short_cpu.c:128-198): the body for the caller's tables
static uint32_t le_compress_with_info(const uint8_t *pIn, uint32_t inSize, const rle8_low_entropy_compress_info_t *info, uint8_t *pOut, uint32_t outSize, uint32_t maxLen)
{
  if (pIn == nullptr || inSize == 0 || info == nullptr || pOut == nullptr || outSize < inSize || !device_ok())
    return 0;
  Rle8mTables ht;
  memset(&ht, 0, sizeof(ht));
  for (uint32_t i = 0; i < 256u; i++)
  {
    const uint8_t flag = ((const uint8_t *)info->rle)[i] ? 1 : 0;
    ht.rle[i] = flag; ht.order[i] = info->symbolsByProb[i];
    ht.rleBits[i >> 5] |= (uint32_t)flag << (i & 31u);
  }
  ht.listed = info->symbolCount ? info->symbolCount : 255u;
  ht.headerSize = 12u + 33u + ht.listed;                                 // (as k_rle8m_info counts it: an rle8m header of one section)
  const uint32_t H = ht.headerSize - 4u;
  const LePlan p = plan_le(inSize, true);
  const uint64_t cap = 2ull * inSize + 512ull;                           // a body is at most twice its input (every byte a flagged symbol with its code)
  Staging s;
  if (!s.reserve(inSize, cap) || !s.reserve_ws(p.total))
    return 0;
  Rle8mTables *t = (Rle8mTables *)(s.ws + p.offTables);
  if (!s.up(pIn, inSize) || hipMemcpy(t, &ht, sizeof(ht), hipMemcpyHostToDevice) != hipSuccess || zero_async(s.status, 8, nullptr) != hipSuccess)
    return 0;
  // (the cuts need the pieces' run starts: the statistics pass into a scratch table -- the caller's tables in `t` stay as they are)
  Rle8mTables *scratchT = (Rle8mTables *)(s.ws + p.offTmpTables);
  const uint32_t *runStart4 = nullptr;
  if (zero_async(scratchT, sizeof(Rle8mTables), nullptr) != hipSuccess || launch_le_stats(s.in, inSize, scratchT, maxLen, s.ws + p.offStats, nullptr, 32768u, &runStart4) != hipSuccess)
    return 0;
  if (le_encode_pieces(s.in, inSize, t, runStart4, maxLen, s.out, cap, s.ws, p, s.status, nullptr) != HSRLE_OK)
    return 0;
  uint32_t status = 1, size = 0;
  if (!s.words(&status, s.status, 1) || status != 0u || !s.words(&size, s.out, 1) || size < H || size - H > outSize)
    return 0;
  if (size > H && !s.down(pOut, s.out + H, size - H))
    return 0;
  return size - H;
}

// rle8_low_entropy[_short]_decompress_with_info (rle8_low_entropy_cpu.c:930-1022, rle8_low_entropy_short_cpu.c:440-534): the body becomes a stream again --
// header and the tables' symbols in front of it, in device memory -- and takes the way of le_mono_decompress (the decode kernels read their tables from the stream)
static uint32_t le_decompress_with_info(const uint8_t *pIn, const uint8_t *pEnd, const rle8_low_entropy_decompress_info_t *info, uint8_t *pOut, uint32_t expOut)
{
  if (pIn == nullptr || pEnd == nullptr || pEnd < pIn || info == nullptr || pOut == nullptr || expOut == 0 || !device_ok())
    return 0;
  const uint64_t body64 = (uint64_t)(pEnd - pIn);
  constexpr uint32_t dataStart = 8u + 33u + 255u;
  if (body64 > 0xFFFFFF00ull - dataStart)
    return 0;
  const uint32_t body = (uint32_t)body64, expIn = dataStart + body;
  uint8_t head[dataStart];
  memset(head, 0, sizeof(head));
  memcpy(head, &expIn, 4); memcpy(head + 4, &expOut, 4);
  for (uint32_t i = 0; i < 256u; i++)
    if (((const uint8_t *)info->rle)[i]) head[8u + (i >> 3)] |= (uint8_t)(1u << (i & 7u));
  head[8u + 32u] = 255u;
  // the symbols in the order of their codes' counts: the inverse of symbolToCount, which must be a permutation (what read_decompress_info produces)
  bool seen[256] = { false };
  for (uint32_t sym = 0; sym < 256u; sym++)
  {
    const uint32_t c = info->symbolToCount[sym];
    if (seen[c]) return 0;
    seen[c] = true;
    if (c < 255u) head[8u + 33u + c] = (uint8_t)sym;
  }
  const uint64_t many = plan_le(body, false).total, one = plan_le(body, false, expIn + 128u).total;
  Staging s;
  if (!s.reserve(expIn, expOut) || !s.reserve_ws(many > one ? many : one) || !s.up(head, dataStart) || !s.up(pIn, body, dataStart, 128))
    return 0;
  if (le_decode_attempts(s.in, expIn, dataStart, expOut, s.out, expOut, s.ws, s.wsSize, s.status, nullptr) != HSRLE_OK || !s.down(pOut, s.out, expOut))
    return 0;
  return expOut;
}

} // namespace hsrle
