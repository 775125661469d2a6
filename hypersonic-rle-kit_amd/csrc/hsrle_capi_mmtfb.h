// hsrle_capi_mmtfb.h -- part of hsrle_capi.hip: C ABI of the rle8_mmtf128 BLOCK CONTAINER (include/hsrle.h section 5): many independent rle8_mmtf128 streams
// per call.  The container's layout, its header check and the blocks-in-flight rule are those of the rle8_sh block container (hsrle_capi_shb.h) under the
// magic "HSRLEMFB".  The plan is made here on the host: one block's slot times the blocks in flight; inst_rle8mmtfb.hip launches the groups (kernels:
// hsrle_rle8mmtfb.hip.h).  No kernel here.  The host-pointer functions take the staged trip of hsrle_capi_host.h.
#pragma once
#include "hsrle_capi_mmtf.h"
#include "hsrle_capi_shb.h"

namespace hsrle {

static std::atomic<uint32_t> g_mfbInFlight{ 0 };
static const char kMfbMagic[8] = { 'H', 'S', 'R', 'L', 'E', 'M', 'F', 'B' };
constexpr uint64_t kMfbStreamSlack = 13u;   // inSize + 13 always suffices for one stream (include/hsrle.h, rle8_mmtf128)

// `blocks`: how many blocks the call handles (a decode may take a range of the container's)
static bool rle8mmtfb_plan(uint64_t size, uint32_t B, uint64_t blocks, MfbPlan &p)
{
  const uint64_t all = size == 0u || !shb_valid_block(B) ? 0u : shb_block_count(size, B);
  if (all == 0u || all > 0xFFFFFFFFull || blocks == 0u || blocks > all)
    return false;
  const uint32_t fly = shb_in_flight(g_mfbInFlight.load(), B), tuning = g_rle8MmtfSpanRows.load(), rows = B / 16u;
  p.size = size;
  p.blockSize = B;
  p.blockCount = (uint32_t)all;
  p.inFlight = blocks < fly ? (uint32_t)blocks : fly;
  p.SP = tuning == 0u || tuning > 64u ? 64u : tuning;
  p.maxRec = rows + 1u;   // a record per non-null packet, and such a packet holds a row
  const uint64_t spans = (rows + p.SP - 1u) / p.SP;
  p.offRanks = 256u;
  p.offA = p.offRanks + align_up((uint64_t)B + 16u, 256);
  p.offB = p.offA + align_up(16u * spans, 256);
  p.encSlot = p.offB + align_up(16u * spans, 256);
  p.decSlot = p.offA + align_up(16ull * p.maxRec, 256);
  return true;
}

static uint64_t rle8mmtfb_bound(uint64_t size, uint32_t B)
{
  const uint64_t blocks = size == 0u || !shb_valid_block(B) ? 0u : shb_block_count(size, B);
  if (blocks == 0u || blocks > 0xFFFFFFFFull)
    return 0u;
  return shb_table_end(blocks) + size + blocks * kMfbStreamSlack + kShbPadBytes;
}

}   // namespace hsrle

extern "C" {

void hsrle_rle8_mmtf128_blocks_tuning(uint32_t blocksInFlight) { g_mfbInFlight.store(blocksInFlight); }

uint64_t hsrle_rle8_mmtf128_blocks_bound(uint64_t inSize, uint32_t blockSize) { return rle8mmtfb_bound(inSize, blockSize == 0u ? kShbBlockDefault : blockSize); }

uint64_t hsrle_rle8_mmtf128_blocks_workspace_size(int decode, uint64_t inSize, uint32_t blockSize)
{
  MfbPlan p;
  const uint32_t B = blockSize == 0u ? kShbBlockDefault : blockSize;
  if (inSize == 0u || !shb_valid_block(B) || !rle8mmtfb_plan(inSize, B, shb_block_count(inSize, B), p))
    return 0u;
  return 512u + (uint64_t)p.inFlight * (decode != 0 ? p.decSlot : p.encSlot);   // (256: the start is rounded up; 256: the call's own words)
}

int hsrle_rle8_mmtf128_blocks_info_host(const void *pContainer, uint64_t containerSize, hsrle_rle8_sh_blocks_info_t *pInfo)
{
  if (!pContainer || !pInfo || containerSize < kShbHeaderBytes) return HSRLE_ERR_ARGUMENT;
  return shb_check_info(kMfbMagic, (const uint8_t *)pContainer, containerSize, pInfo);
}

int hsrle_rle8_mmtf128_blocks_info_dev(const void *dContainer, uint64_t containerSize, hsrle_rle8_sh_blocks_info_t *pInfo, void *stream)
{
  if (!dContainer || !pInfo || containerSize < kShbHeaderBytes) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  uint8_t h[64];
  if (hipMemcpyAsync(h, dContainer, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  return shb_check_info(kMfbMagic, h, containerSize, pInfo);
}

int hsrle_rle8_mmtf128_compress_blocks_dev_async(const void *dIn, uint64_t inSize, uint32_t blockSize, void *dOut, uint64_t outCapacity, uint64_t *dOutSize, uint32_t *dStatus,
                                                 void *dWorkspace, uint64_t workspaceSize, void *stream)
{
  MfbPlan p;
  const uint32_t B = blockSize == 0u ? kShbBlockDefault : blockSize;
  if (dIn == nullptr || dOut == nullptr || dOutSize == nullptr || dStatus == nullptr || dWorkspace == nullptr || inSize == 0u || !shb_valid_block(B) ||
      !rle8mmtfb_plan(inSize, B, shb_block_count(inSize, B), p))
    return HSRLE_ERR_ARGUMENT;
  if (ranges_overlap(dIn, inSize, dOut, outCapacity) || !word_aligned(dOutSize, 8) || !word_aligned(dStatus, 4))
    return HSRLE_ERR_ARGUMENT;
  if (outCapacity < shb_table_end(p.blockCount) + kShbPadBytes || workspaceSize < 512u + (uint64_t)p.inFlight * p.encSlot)
    return HSRLE_ERR_CAPACITY;
  return rle8mmtfb_compress_enqueue(p, (const uint8_t *)dIn, (uint8_t *)dOut, outCapacity, dOutSize, dStatus, workspace_start(dWorkspace), (hipStream_t)stream) == hipSuccess
           ? HSRLE_OK
           : HSRLE_ERR_DEVICE;
}

int hsrle_rle8_mmtf128_decompress_blocks_dev_async(const void *dContainer, const hsrle_rle8_sh_blocks_info_t *info, uint32_t firstBlock, uint32_t blockCount, void *dOut,
                                                   uint64_t outCapacity, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize, void *stream)
{
  MfbPlan p;
  if (dContainer == nullptr || info == nullptr || dOut == nullptr || dStatus == nullptr || dWorkspace == nullptr || !shb_info_consistent(*info))
    return HSRLE_ERR_ARGUMENT;
  if (blockCount == 0u || (uint64_t)firstBlock + blockCount > info->blockCount || !rle8mmtfb_plan(info->uncompressedSize, info->blockSize, blockCount, p))
    return HSRLE_ERR_ARGUMENT;
  if (outCapacity < info->uncompressedSize)
    return HSRLE_ERR_CAPACITY;
  if (ranges_overlap(dContainer, info->totalSize, dOut, info->uncompressedSize) || !word_aligned(dStatus, 4))
    return HSRLE_ERR_ARGUMENT;
  if (workspaceSize < 512u + (uint64_t)p.inFlight * p.decSlot)
    return HSRLE_ERR_CAPACITY;
  return rle8mmtfb_decompress_enqueue(p, (const uint8_t *)dContainer, info->payloadSize, firstBlock, blockCount, (uint8_t *)dOut, dStatus, workspace_start(dWorkspace),
                                      (hipStream_t)stream) == hipSuccess
           ? HSRLE_OK
           : HSRLE_ERR_DEVICE;
}

int hsrle_rle8_mmtf128_compress_blocks_host(const void *pIn, uint64_t inSize, uint32_t blockSize, void *pOut, uint64_t outCapacity, uint64_t *pContainerSize)
{
  if (!pIn || !pOut || inSize == 0u) return HSRLE_ERR_ARGUMENT;
  const uint64_t bound = hsrle_rle8_mmtf128_blocks_bound(inSize, blockSize), need = hsrle_rle8_mmtf128_blocks_workspace_size(0, inSize, blockSize);
  if (bound == 0u || need == 0u) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  uint64_t total = 0;
  // (the status words are 64-byte aligned: the size word is their first 8 bytes, the status the word behind)
  const int rc = staged_call(
    pIn, inSize, bound, need, pOut, 3u,
    [&](Staging &s) { return hsrle_rle8_mmtf128_compress_blocks_dev_async(s.in, inSize, blockSize, s.out, bound, (uint64_t *)s.status, s.status + 2, s.ws, s.wsSize, nullptr); },
    [&](const uint32_t *h, uint64_t &n) {
      n = (uint64_t)h[0] | (uint64_t)h[1] << 32;
      if (h[2] != HSRLE_RLE8_MMTF_DONE || n == 0u) return (int)HSRLE_ERR_DEVICE;   // (the bound always suffices)
      return n > outCapacity ? (int)HSRLE_ERR_CAPACITY : (int)HSRLE_OK;
    },
    &total);
  if (rc == HSRLE_OK && pContainerSize) *pContainerSize = total;
  return rc;
}

int hsrle_rle8_mmtf128_decompress_blocks_host(const void *pContainer, uint64_t containerSize, void *pOut, uint64_t outCapacity, uint64_t *pUncompressedSize)
{
  hsrle_rle8_sh_blocks_info_t info;
  int rc = hsrle_rle8_mmtf128_blocks_info_host(pContainer, containerSize, &info);
  if (rc != HSRLE_OK) return rc;
  if (!pOut || outCapacity < info.uncompressedSize) return HSRLE_ERR_CAPACITY;
  const uint64_t need = hsrle_rle8_mmtf128_blocks_workspace_size(1, info.uncompressedSize, info.blockSize);
  if (need == 0u) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  uint64_t size = 0;
  rc = staged_call(
    pContainer, info.totalSize, info.uncompressedSize, need, pOut, 1u,
    [&](Staging &s) { return hsrle_rle8_mmtf128_decompress_blocks_dev_async(s.in, &info, 0u, info.blockCount, s.out, info.uncompressedSize, s.status, s.ws, s.wsSize, nullptr); },
    [&](const uint32_t *h, uint64_t &n) { n = info.uncompressedSize; return h[0] != HSRLE_RLE8_MMTF_DONE ? (int)HSRLE_ERR_FORMAT : (int)HSRLE_OK; }, &size);
  if (rc == HSRLE_OK && pUncompressedSize) *pUncompressedSize = size;
  return rc;
}

}   // extern "C"
