// hsrle_capi_shb.h -- part of hsrle_capi.hip: C ABI of the rle8_sh BLOCK CONTAINER (include/hsrle.h section 5): many independent rle8_sh streams per call.
// The plan is made here on the host: one block's single-stream plans (hsrle_capi_sh.h) times the blocks in flight; inst_rle8shb.hip launches the groups
// (kernels: hsrle_rle8shb.hip.h).  No kernel here.  The host-pointer functions take the staged trip of hsrle_capi_host.h.
#pragma once
#include "hsrle_capi_sh.h"

namespace hsrle {

static std::atomic<uint32_t> g_shbInFlight{ 0 };
constexpr uint32_t kShbBlockDefault = 4096u, kShbBlockMin = 128u, kShbBlockMax = 1u << 20;
constexpr uint64_t kShbHeaderBytes = 64u, kShbPadBytes = 32u;
// Blocks in flight by default: 32 MiB of input per group, at least 256 and at most 8 192 blocks.  A block is ONE wave in every pass; 256 CUs hold 8 192
// waves at their full 32 per CU, so 8 192 blocks of 4 KiB fill the device once, and their decode slots (24 bytes per output byte) stay under 1 GiB.
constexpr uint32_t kShbInFlightMax = 8192u, kShbInFlightMin = 256u;
constexpr uint64_t kShbGroupBytes = 32ull << 20;

static const char kShbMagic[8] = { 'H', 'S', 'R', 'L', 'E', 'S', 'H', 'B' };

static bool shb_valid_block(uint32_t B) { return B >= kShbBlockMin && B <= kShbBlockMax && B % 128u == 0u; }
static uint64_t shb_block_count(uint64_t size, uint32_t B) { return (size + B - 1u) / B; }
static uint64_t shb_table_end(uint64_t blocks) { return kShbHeaderBytes + 8ull * (blocks + 1u); }

// `t`: the family's tuning value (0 = the default)
static uint32_t shb_in_flight(uint32_t t, uint32_t B)
{
  if (t != 0u) return t;
  const uint64_t d = kShbGroupBytes / B;
  return d > kShbInFlightMax ? kShbInFlightMax : (d < kShbInFlightMin ? kShbInFlightMin : (uint32_t)d);
}

// `blocks`: how many blocks the call handles (a decode may take a range of the container's)
static bool rle8shb_plan(uint64_t size, uint32_t B, uint64_t blocks, ShbPlan &p)
{
  const uint64_t all = size == 0u || !shb_valid_block(B) ? 0u : shb_block_count(size, B);
  if (all == 0u || all > 0xFFFFFFFFull || blocks == 0u || blocks > all || !rle8sh_enc_plan(B, p.enc) || !rle8sh_plan(B, p.dec))
    return false;
  const uint32_t fly = shb_in_flight(g_shbInFlight.load(), B);
  p.size = size;
  p.blockSize = B;
  p.blockCount = (uint32_t)all;
  p.inFlight = blocks < fly ? (uint32_t)blocks : fly;
  return true;
}

static uint64_t rle8shb_bound(uint64_t size, uint32_t B)
{
  const uint64_t blocks = size == 0u || !shb_valid_block(B) ? 0u : shb_block_count(size, B);
  if (blocks == 0u || blocks > 0xFFFFFFFFull)
    return 0u;
  return shb_table_end(blocks) + (blocks - 1u) * rle8sh_capacity(B) + rle8sh_capacity(size - (blocks - 1u) * B) + kShbPadBytes;
}

// (both stream-block containers: the same header lines under the family's own magic)
static int shb_check_info(const char magic[8], const uint8_t h[64], uint64_t containerSize, hsrle_rle8_sh_blocks_info_t *info)
{
  uint32_t version, reserved, B, blocks;
  uint64_t size, payload, total;
  memcpy(&version, h + 8, 4); memcpy(&reserved, h + 12, 4); memcpy(&size, h + 16, 8); memcpy(&B, h + 24, 4); memcpy(&blocks, h + 28, 4);
  memcpy(&payload, h + 32, 8); memcpy(&total, h + 40, 8);
  if (memcmp(h, magic, 8) != 0 || version != 1u || reserved != 0u)
    return HSRLE_ERR_FORMAT;
  for (int k = 48; k < 64; k++)
    if (h[k] != 0u) return HSRLE_ERR_FORMAT;
  if (!shb_valid_block(B) || size == 0u || shb_block_count(size, B) != blocks)
    return HSRLE_ERR_FORMAT;
  if (payload > containerSize || total != shb_table_end(blocks) + payload + kShbPadBytes || total > containerSize)
    return HSRLE_ERR_FORMAT;
  info->uncompressedSize = size; info->blockSize = B; info->blockCount = blocks; info->payloadSize = payload; info->totalSize = total;
  return HSRLE_OK;
}

// an info a caller hands to the decoder: the same relations, without the bytes
static bool shb_info_consistent(const hsrle_rle8_sh_blocks_info_t &i)
{
  return shb_valid_block(i.blockSize) && i.uncompressedSize != 0u && shb_block_count(i.uncompressedSize, i.blockSize) == i.blockCount &&
         i.payloadSize <= i.totalSize && i.totalSize == shb_table_end(i.blockCount) + i.payloadSize + kShbPadBytes;
}

}   // namespace hsrle

extern "C" {

void hsrle_rle8_sh_blocks_tuning(uint32_t blocksInFlight) { g_shbInFlight.store(blocksInFlight); }

uint64_t hsrle_rle8_sh_blocks_bound(uint64_t inSize, uint32_t blockSize) { return rle8shb_bound(inSize, blockSize == 0u ? kShbBlockDefault : blockSize); }

uint64_t hsrle_rle8_sh_blocks_workspace_size(int decode, uint64_t inSize, uint32_t blockSize)
{
  ShbPlan p;
  const uint32_t B = blockSize == 0u ? kShbBlockDefault : blockSize;
  if (inSize == 0u || !shb_valid_block(B) || !rle8shb_plan(inSize, B, shb_block_count(inSize, B), p))
    return 0u;
  return 512u + (uint64_t)p.inFlight * (decode != 0 ? p.dec.total : p.enc.total);   // (256: the start is rounded up; 256: the call's own words)
}

int hsrle_rle8_sh_blocks_info_host(const void *pContainer, uint64_t containerSize, hsrle_rle8_sh_blocks_info_t *pInfo)
{
  if (!pContainer || !pInfo || containerSize < kShbHeaderBytes) return HSRLE_ERR_ARGUMENT;
  return shb_check_info(kShbMagic, (const uint8_t *)pContainer, containerSize, pInfo);
}

int hsrle_rle8_sh_blocks_info_dev(const void *dContainer, uint64_t containerSize, hsrle_rle8_sh_blocks_info_t *pInfo, void *stream)
{
  if (!dContainer || !pInfo || containerSize < kShbHeaderBytes) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  uint8_t h[64];
  if (hipMemcpyAsync(h, dContainer, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  return shb_check_info(kShbMagic, h, containerSize, pInfo);
}

int hsrle_rle8_sh_compress_blocks_dev_async(const void *dIn, uint64_t inSize, uint32_t blockSize, void *dOut, uint64_t outCapacity, uint64_t *dOutSize, uint32_t *dStatus,
                                            void *dWorkspace, uint64_t workspaceSize, void *stream)
{
  ShbPlan p;
  const uint32_t B = blockSize == 0u ? kShbBlockDefault : blockSize;
  if (dIn == nullptr || dOut == nullptr || dOutSize == nullptr || dStatus == nullptr || dWorkspace == nullptr || inSize == 0u || !shb_valid_block(B) ||
      !rle8shb_plan(inSize, B, shb_block_count(inSize, B), p))
    return HSRLE_ERR_ARGUMENT;
  if (ranges_overlap(dIn, inSize, dOut, outCapacity) || !word_aligned(dOutSize, 8) || !word_aligned(dStatus, 4))
    return HSRLE_ERR_ARGUMENT;
  if (outCapacity < shb_table_end(p.blockCount) + kShbPadBytes || workspaceSize < 512u + (uint64_t)p.inFlight * p.enc.total)
    return HSRLE_ERR_CAPACITY;
  return rle8shb_compress_enqueue(p, (const uint8_t *)dIn, (uint8_t *)dOut, outCapacity, dOutSize, dStatus, workspace_start(dWorkspace), (hipStream_t)stream) == hipSuccess
           ? HSRLE_OK
           : HSRLE_ERR_DEVICE;
}

int hsrle_rle8_sh_decompress_blocks_dev_async(const void *dContainer, const hsrle_rle8_sh_blocks_info_t *info, uint32_t firstBlock, uint32_t blockCount, void *dOut,
                                              uint64_t outCapacity, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize, void *stream)
{
  ShbPlan p;
  if (dContainer == nullptr || info == nullptr || dOut == nullptr || dStatus == nullptr || dWorkspace == nullptr || !shb_info_consistent(*info))
    return HSRLE_ERR_ARGUMENT;
  if (blockCount == 0u || (uint64_t)firstBlock + blockCount > info->blockCount || !rle8shb_plan(info->uncompressedSize, info->blockSize, blockCount, p))
    return HSRLE_ERR_ARGUMENT;
  if (outCapacity < info->uncompressedSize)
    return HSRLE_ERR_CAPACITY;
  if (ranges_overlap(dContainer, info->totalSize, dOut, info->uncompressedSize) || !word_aligned(dStatus, 4))
    return HSRLE_ERR_ARGUMENT;
  if (workspaceSize < 512u + (uint64_t)p.inFlight * p.dec.total)
    return HSRLE_ERR_CAPACITY;
  return rle8shb_decompress_enqueue(p, (const uint8_t *)dContainer, info->payloadSize, firstBlock, blockCount, (uint8_t *)dOut, dStatus, workspace_start(dWorkspace),
                                    (hipStream_t)stream) == hipSuccess
           ? HSRLE_OK
           : HSRLE_ERR_DEVICE;
}

int hsrle_rle8_sh_compress_blocks_host(const void *pIn, uint64_t inSize, uint32_t blockSize, void *pOut, uint64_t outCapacity, uint64_t *pContainerSize)
{
  if (!pIn || !pOut || inSize == 0u) return HSRLE_ERR_ARGUMENT;
  const uint64_t bound = hsrle_rle8_sh_blocks_bound(inSize, blockSize), need = hsrle_rle8_sh_blocks_workspace_size(0, inSize, blockSize);
  if (bound == 0u || need == 0u) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  uint64_t total = 0;
  // (the status words are 64-byte aligned: the size word is their first 8 bytes, the status the word behind)
  const int rc = staged_call(
    pIn, inSize, bound, need, pOut, 3u,
    [&](Staging &s) { return hsrle_rle8_sh_compress_blocks_dev_async(s.in, inSize, blockSize, s.out, bound, (uint64_t *)s.status, s.status + 2, s.ws, s.wsSize, nullptr); },
    [&](const uint32_t *h, uint64_t &n) {
      n = (uint64_t)h[0] | (uint64_t)h[1] << 32;
      if (h[2] != HSRLE_RLE8_SH_DONE || n == 0u) return (int)HSRLE_ERR_DEVICE;   // (the bound always suffices)
      return n > outCapacity ? (int)HSRLE_ERR_CAPACITY : (int)HSRLE_OK;
    },
    &total);
  if (rc == HSRLE_OK && pContainerSize) *pContainerSize = total;
  return rc;
}

int hsrle_rle8_sh_decompress_blocks_host(const void *pContainer, uint64_t containerSize, void *pOut, uint64_t outCapacity, uint64_t *pUncompressedSize)
{
  hsrle_rle8_sh_blocks_info_t info;
  int rc = hsrle_rle8_sh_blocks_info_host(pContainer, containerSize, &info);
  if (rc != HSRLE_OK) return rc;
  if (!pOut || outCapacity < info.uncompressedSize) return HSRLE_ERR_CAPACITY;
  const uint64_t need = hsrle_rle8_sh_blocks_workspace_size(1, info.uncompressedSize, info.blockSize);
  if (need == 0u) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  uint64_t size = 0;
  rc = staged_call(
    pContainer, info.totalSize, info.uncompressedSize, need, pOut, 1u,
    [&](Staging &s) { return hsrle_rle8_sh_decompress_blocks_dev_async(s.in, &info, 0u, info.blockCount, s.out, info.uncompressedSize, s.status, s.ws, s.wsSize, nullptr); },
    [&](const uint32_t *h, uint64_t &n) { n = info.uncompressedSize; return h[0] != HSRLE_RLE8_SH_DONE ? (int)HSRLE_ERR_FORMAT : (int)HSRLE_OK; }, &size);
  if (rc == HSRLE_OK && pUncompressedSize) *pUncompressedSize = size;
  return rc;
}

}   // extern "C"
