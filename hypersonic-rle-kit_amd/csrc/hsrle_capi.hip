// hsrle_capi.hip -- the C ABI of libhsrle_hip.so (include/hsrle.h): drop-in rle.h entry points, the device-resident
// block container API, container assembly kernels (size scan + slot compaction) and the synthetic workload generator.
// What a codec id means is said once, in hsrle_codecs.h: nothing here compares an id with a number.
//
// ONE translation unit (it alone embeds HSRLE_BUILD_ID), cut into the hsrle_capi_*.h parts below; this file holds the exported functions only.
// The order of the kernel headers and of the parts is the order of the kernels in the device code object: keep it.
// Host code here is plain C-style C++ behind `extern "C"`; no torch types, no CPU codec.  If no HIP device is usable
// every entry point fails loudly (0 / HSRLE_ERR_DEVICE) -- there is no fallback path.
#include "../../include/hsrle.h"

#include "hsrle_common.hip.h"
#include "hsrle_launch.h"
#include "hsrle_index.hip.h"
#include "hsrle_expand.hip.h"
#include "hsrle_mono_encode.hip.h"
#ifdef HSRLE_EXPERIMENTS
#include "experiments/hsrle_encode8w.hip.h"
#endif
#include "hsrle_rle8m.hip.h"

#include <string.h>

#include "hsrle_capi_host.h"                // launch tables, size helpers, device state and scratch, Staging
#include "hsrle_capi_kernels.h"             // scan / compact / finish / hash / synth kernels, scan_sizes
#include "hsrle_capi_mono_decode.h"         // MonoPlan, stream header, the decode sequence and its repair loop
#include "hsrle_capi_mono_index.h"          // persistent index: header, tag and gate kernels
#include "hsrle_capi_container.h"           // Workspace, the container encode paths, block / split decode
#include "hsrle_capi_mono_encode.h"         // MonoEncPlan, mono_encode_dev
#include "hsrle_capi_low_entropy.h"         // rle8m and the unsectioned low-entropy codec on device pointers
#include "hsrle_capi_dropin.h"              // the host-pointer functions of all families

// ====================================================================================================================
using namespace hsrle;

#include "hsrle_capi_mmtf.h"                // the mmtf / bitmmtf transforms and rle8_mmtf128: plans, their C ABI, their host-pointer functions
#include "hsrle_capi_sh.h"                  // rle8_sh, both directions: plans, C ABI, host-pointer functions
#include "hsrle_capi_shb.h"                 // the rle8_sh block container: many independent rle8_sh streams per call
#include "hsrle_capi_mmtfb.h"               // the rle8_mmtf128 block container: the same container of rle8_mmtf128 streams

extern "C" {

int hsrle_codec_from_name(const char *name)
{
  if (!name) return -1;
  for (int k = 0; k < kCodecCount; k++)
    if (strcmp(name, kCodecs[k].name) == 0) return k;
  return -1;
}

const char *hsrle_codec_name(int codec) { return (codec >= 0 && codec < kCodecCount) ? kCodecs[codec].name : nullptr; }

const char *hsrle_status_string(int s)
{
  switch (s)
  {
  case HSRLE_OK: return "ok";
  case HSRLE_ERR_ARGUMENT: return "invalid argument";
  case HSRLE_ERR_CAPACITY: return "buffer too small";
  case HSRLE_ERR_FORMAT: return "malformed container or stream";
  case HSRLE_ERR_DEVICE: return "no usable HIP device / HIP runtime error";
  case HSRLE_ERR_UNSUPPORTED: return "codec not available in this build";
  }
  return "unknown";
}

const char *hsrle_version(void) { return "hsrle-hip 0.1 (gfx950)"; }

uint32_t hsrle_suggest_block_size(uint64_t inSize)
{
  if (inSize >= 65536ull * 4096ull) return 4096u;
  if (inSize >= 65536ull * 2048ull) return 2048u;
  return 1024u;
}

int hsrle_kernel_waves_per_cu(int codec, int decode)
{
  if (codec < 0 || codec >= kCodecCount)
    return 0;
  init_tables();
  int n = 0;
  if (decode) { DecodeArgs a{}; a.residentWorkgroups = &n; if (g_launch[codec].dec(a, nullptr) != hipSuccess) return 0; }
  else { EncodeArgs a{}; a.residentWorkgroups = &n; if (g_launch[codec].enc(a, nullptr) != hipSuccess) return 0; }
  return n;
}

int hsrle_scratch_retention(uint64_t bytes)
{
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  g_scratchRetention.store(bytes);
  hipMemPool_t pool = device_pool();
  if (pool == nullptr) return HSRLE_ERR_UNSUPPORTED;
  uint64_t keep = bytes;
  return hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

int hsrle_trim(void)
{
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  hipMemPool_t pool = device_pool();
  if (pool == nullptr) return HSRLE_OK;
  return hipMemPoolTrimTo(pool, 0) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

int hsrle_experiments_enabled(void) { return kExperiments ? 1 : 0; }

int hsrle_encode_path(int codec, uint64_t uncompressedSize, uint32_t blockSize)
{
  if (codec < 0 || codec >= kCodecCount || uncompressedSize == 0 || !valid_block_size(blockSize)) return -1;
  const EncodeChoice ec = encode_choice_of(codec, uncompressedSize, blockSize, encode_knobs().generic);   // (the workspace every caller has: include/hsrle.h)
  if (ec.path == ENC_PP || ec.path == ENC_PPW) return HSRLE_PATH_POSITION_PARALLEL;
  return ec.path == ENC_SPLIT ? HSRLE_PATH_SPLIT : (ec.runList ? HSRLE_PATH_RUN_LIST : HSRLE_PATH_RING);
}

int hsrle_decode_ring(int codec, uint64_t uncompressedSize, uint64_t payloadSize)
{
  if (codec < 0 || codec >= kCodecCount) return -1;
  return decode_ring_small(kCodecs[codec], uncompressedSize, payloadSize + HSRLE_CONTAINER_TAIL_PAD) ? 64 : 128;   // (what DecodeArgs::payloadEnd - payload is for this container)
}

#ifndef HSRLE_BUILD_ID
#define HSRLE_BUILD_ID "unknown"
#endif
const char *hsrle_build_id(void) { return HSRLE_BUILD_ID; }

int hsrle_device_count(void)
{
  int n = 0;
  return (hipGetDeviceCount(&n) == hipSuccess) ? n : 0;
}

// device-resident forms (benchmarks, pipelines that keep the data on the GPU).  variant: bit 0 the Short form, bit 1 only_max_frequency.
uint64_t hsrle_low_entropy_workspace_size(uint32_t inSize) { return inSize == 0 ? 0 : plan_le(inSize, true).total; }
int hsrle_low_entropy_compress_dev_async(const void *dIn, uint32_t inSize, int variant, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize, uint32_t *dStatus, void *stream)
{
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  if (variant < 0 || variant > 3) return HSRLE_ERR_ARGUMENT;
  return le_encode_async(dIn, inSize, dOut, outCapacity, dWorkspace, workspaceSize, dStatus, (variant & 1) ? 32u : 255u, (variant & 2) ? 1u : 0u, (hipStream_t)stream);
}
// reads the stream's header (synchronises the stream once), decodes, reads the verdict: HSRLE_OK / HSRLE_ERR_FORMAT / ...
int hsrle_low_entropy_decompress_dev(const void *dStream, uint64_t streamSize, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize, uint32_t *pUncompressedSize, void *stream)
{
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  if (!dStream || !dOut || !dWorkspace || streamSize < 8u + 33u || workspaceSize < 256u) return HSRLE_ERR_ARGUMENT;
  uint8_t head[48];
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(head, dStream, 48, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return HSRLE_ERR_DEVICE;
  uint32_t expIn, expOut;
  memcpy(&expIn, head, 4); memcpy(&expOut, head + 4, 4);
  uint32_t listed = head[40]; if (listed == 0u) listed = 255u;
  const uint32_t dataStart = 8u + 33u + listed;
  if ((uint64_t)expIn > streamSize || dataStart > expIn || expOut == 0u || expIn > 0xFFFFFF00u) return HSRLE_ERR_FORMAT;   // (the last: the piece arithmetic of le_decode_async is 32 bit, as on the host path)
  if (outCapacity < expOut) return HSRLE_ERR_CAPACITY;
  // (the first 256 bytes of the workspace: the status words; word 2 = the attempts, include/hsrle.h)
  const int rc = le_decode_attempts(dStream, expIn, dataStart, expOut, dOut, outCapacity, (uint8_t *)dWorkspace + 256, workspaceSize - 256, (uint32_t *)dWorkspace, st);
  if (rc == HSRLE_OK && pUncompressedSize) *pUncompressedSize = expOut;
  return rc;
}
uint64_t hsrle_low_entropy_decompress_workspace_size(uint64_t streamSize) { const uint64_t a = plan_le(streamSize, false).total, b = plan_le(streamSize, false, (uint32_t)(streamSize > 0xFFFFFF00ull ? 0xFFFFFF00ull : streamSize) + 128u).total; return 256u + (a > b ? a : b); }

uint32_t rle8_low_entropy_compress_bounds(const uint32_t inSize) { return le_bounds(inSize); }
uint32_t rle8_low_entropy_short_compress_bounds(const uint32_t inSize) { return le_bounds(inSize); }
uint32_t rle8_low_entropy_decompressed_size(const uint8_t *pIn, const uint32_t inSize)
{
  if (pIn == nullptr || inSize < 8u) return 0;                                               // rle8_low_entropy_cpu.c:88-94
  uint32_t v; memcpy(&v, pIn + 4, 4); return v;
}
uint32_t rle8_low_entropy_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return le_mono_compress(pIn, inSize, pOut, outSize, 255u, 0u); }
uint32_t rle8_low_entropy_compress_only_max_frequency(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return le_mono_compress(pIn, inSize, pOut, outSize, 255u, 1u); }
uint32_t rle8_low_entropy_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return le_mono_decompress(pIn, inSize, pOut, outSize); }
uint32_t rle8_low_entropy_short_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return le_mono_compress(pIn, inSize, pOut, outSize, 32u, 0u); }
uint32_t rle8_low_entropy_short_compress_only_max_frequency(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return le_mono_compress(pIn, inSize, pOut, outSize, 32u, 1u); }
uint32_t rle8_low_entropy_short_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return le_mono_decompress(pIn, inSize, pOut, outSize); }

bool rle8_low_entropy_get_compress_info(const uint8_t *pIn, const uint32_t inSize, rle8_low_entropy_compress_info_t *pCompressInfo) { return le_get_info(pIn, inSize, pCompressInfo, 0u); }
bool rle8_low_entropy_get_compress_info_only_max_frequency(const uint8_t *pIn, const uint32_t inSize, rle8_low_entropy_compress_info_t *pCompressInfo) { return le_get_info(pIn, inSize, pCompressInfo, 1u); }
uint32_t rle8_low_entropy_write_compress_info(rle8_low_entropy_compress_info_t *pCompressInfo, uint8_t *pOut, const uint32_t outSize)
{
  // host only (rle8_low_entropy_cpu.c:441-472): 32 flag bytes, the count byte, the symbols (a count of 0 stands for 256 in use: 255 are written)
  if (pCompressInfo == nullptr || pOut == nullptr || outSize < 256u / 8u + 256u + 1u)
    return 0;
  memset(pOut, 0, 32);
  for (uint32_t i = 0; i < 256u; i++)
    if (((const uint8_t *)pCompressInfo->rle)[i]) pOut[i >> 3] |= (uint8_t)(1u << (i & 7u));
  pOut[32] = pCompressInfo->symbolCount;
  const uint32_t listed = pCompressInfo->symbolCount ? pCompressInfo->symbolCount : 255u;
  memcpy(pOut + 33, pCompressInfo->symbolsByProb, listed);
  return 33u + listed;
}
uint32_t rle8_low_entropy_read_decompress_info(const uint8_t *pIn, const uint32_t inSize, rle8_low_entropy_decompress_info_t *pDecompressInfo)
{
  // host only (rle8_low_entropy_cpu.c:545-605): the listed symbols get the counts 0, 1, ... in the order they are listed, the others the counts behind them in
  // ascending order.  (The reference does not look at inSize beyond "not 0"; here a header that does not fit is refused.)
  if (pIn == nullptr || pDecompressInfo == nullptr || inSize < 33u)
    return 0;
  uint32_t listed = pIn[32];
  if (listed == 0u) listed = 255u;
  if (inSize < 33u + listed)
    return 0;
  bool isListed[256] = { false };
  for (uint32_t i = 0; i < 256u; i++) pDecompressInfo->rle[i] = ((pIn[i >> 3] >> (i & 7u)) & 1u) != 0u;
  for (uint32_t i = 0; i < listed; i++) { pDecompressInfo->symbolToCount[pIn[33u + i]] = (uint8_t)i; isListed[pIn[33u + i]] = true; }
  uint32_t next = listed;
  for (uint32_t sym = 0; sym < 256u; sym++)
    if (!isListed[sym]) pDecompressInfo->symbolToCount[sym] = (uint8_t)next++;
  return 33u + listed;
}
uint32_t rle8_low_entropy_compress_with_info(const uint8_t *pIn, const uint32_t inSize, const rle8_low_entropy_compress_info_t *pCompressInfo, uint8_t *pOut, const uint32_t outSize) { return le_compress_with_info(pIn, inSize, pCompressInfo, pOut, outSize, 255u); }
uint32_t rle8_low_entropy_short_compress_with_info(const uint8_t *pIn, const uint32_t inSize, const rle8_low_entropy_compress_info_t *pCompressInfo, uint8_t *pOut, const uint32_t outSize) { return le_compress_with_info(pIn, inSize, pCompressInfo, pOut, outSize, 32u); }
uint32_t rle8_low_entropy_decompress_with_info(const uint8_t *pIn, const uint8_t *pEnd, const rle8_low_entropy_decompress_info_t *pDecompressInfo, uint8_t *pOut, const uint32_t expectedOutSize) { return le_decompress_with_info(pIn, pEnd, pDecompressInfo, pOut, expectedOutSize); }
uint32_t rle8_low_entropy_short_decompress_with_info(const uint8_t *pIn, const uint8_t *pEnd, const rle8_low_entropy_decompress_info_t *pDecompressInfo, uint8_t *pOut, const uint32_t expectedOutSize) { return le_decompress_with_info(pIn, pEnd, pDecompressInfo, pOut, expectedOutSize); }

// ---- rle8m: names of the reference's GPU decode path (src/rle.h:464-466) and of its CPU twin (src/rle.h:63) ----
bool rle8m_opencl_init(const size_t inputDataSize, const size_t outputDataSize, const size_t maxSubsectionCount)
{
  (void)inputDataSize; (void)outputDataSize; (void)maxSubsectionCount;    // device buffers are (re)sized by the call that needs them
  return device_ok();
}
void rle8m_opencl_destroy(void) {}
uint32_t rle8m_opencl_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return rle8m_mono_decompress(pIn, inSize, pOut, outSize); }
uint32_t rle8m_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return rle8m_mono_decompress(pIn, inSize, pOut, outSize); }

uint32_t rle8m_compress_bounds(const uint32_t subSections, const uint32_t inSize) { return rle8m_bounds(subSections, inSize); }
uint32_t rle8m_compress(const uint32_t subSections, const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return rle8m_mono_compress(subSections, pIn, inSize, pOut, outSize); }

uint64_t hsrle_rle8m_compress_workspace_size(uint32_t inSize, uint32_t sections) { return (inSize == 0 || sections == 0) ? 0 : plan_rle8m(inSize, sections).total; }

int hsrle_rle8m_compress_dev_async(const void *dIn, uint32_t inSize, uint32_t sections, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize, uint32_t *dStatus, void *stream)
{
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  return rle8m_encode_async(dIn, inSize, sections, dOut, outCapacity, dWorkspace, workspaceSize, dStatus, (hipStream_t)stream);
}

int hsrle_rle8m_info_dev(const void *dStream, uint64_t streamSize, hsrle_rle8m_info_t *pInfo, void *stream)
{
  if (!dStream || !pInfo || streamSize < 12) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  uint32_t h[3];
  if (hipMemcpyAsync(h, dStream, 12, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  if (h[0] > streamSize || h[2] == 0 || h[0] < 12ull + 4ull * (h[2] - 1) + 33ull) return HSRLE_ERR_FORMAT;
  pInfo->compressedSize = h[0]; pInfo->uncompressedSize = h[1]; pInfo->sections = h[2];
  return HSRLE_OK;
}

int hsrle_rle8m_decompress_dev_async(const void *dStream, const hsrle_rle8m_info_t *info, void *dOut, uint64_t outCapacity, uint32_t *dStatus, void *stream)
{
  if (!info) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  return rle8m_decode_async(dStream, info->compressedSize, info->uncompressedSize, info->sections, dOut, outCapacity, dStatus, (hipStream_t)stream);
}

uint32_t rle_compress_bounds(const uint32_t inSize) { return bounds32(inSize); }
uint32_t rle_decompress_additional_size(void) { return 128; }

uint32_t hsrle_compress_mono(int codec, const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize) { return mono_compress(codec, pIn, inSize, pOut, outSize); }
uint32_t hsrle_decompress_mono(int codec, const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize) { return mono_decompress(codec, pIn, inSize, pOut, outSize); }

#define HSRLE_DEF_PAIR(name, id)                                                                                                                             \
  uint32_t name##_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mono_compress(id, pIn, inSize, pOut, outSize); } \
  uint32_t name##_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mono_decompress(id, pIn, inSize, pOut, outSize); }
#define HSRLE_DEF_WIDTH(W)                                                                                                                                  \
  HSRLE_DEF_PAIR(rle##W##_sym, codec_id(PLAIN, W / 8, 1)) HSRLE_DEF_PAIR(rle##W##_sym_packed, codec_id(PACKED, W / 8, 1))                                     \
  HSRLE_DEF_PAIR(rle##W##_3symlut_sym, codec_id(LUT3, W / 8, 1)) HSRLE_DEF_PAIR(rle##W##_7symlut_sym, codec_id(LUT7, W / 8, 1))                               \
  HSRLE_DEF_PAIR(rle##W##_byte, codec_id(PLAIN, W / 8, 0)) HSRLE_DEF_PAIR(rle##W##_byte_packed, codec_id(PACKED, W / 8, 0))                                   \
  HSRLE_DEF_PAIR(rle##W##_3symlut_byte, codec_id(LUT3, W / 8, 0)) HSRLE_DEF_PAIR(rle##W##_7symlut_byte, codec_id(LUT7, W / 8, 0))

uint32_t rle8_multi_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mono_compress(HSRLE_RLE8_MULTI, pIn, inSize, pOut, outSize); }
uint32_t rle8_single_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mono_compress(HSRLE_RLE8_SINGLE, pIn, inSize, pOut, outSize); }
uint32_t rle8_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mono_decompress(HSRLE_RLE8_MULTI, pIn, inSize, pOut, outSize); }
uint32_t rle8_packed_multi_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mono_compress(HSRLE_RLE8_PACKED_MULTI, pIn, inSize, pOut, outSize); }
uint32_t rle8_packed_single_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mono_compress(HSRLE_RLE8_PACKED_SINGLE, pIn, inSize, pOut, outSize); }
uint32_t rle8_packed_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mono_decompress(HSRLE_RLE8_PACKED_MULTI, pIn, inSize, pOut, outSize); }
HSRLE_DEF_PAIR(rle8_3symlut, HSRLE_RLE8_3SYMLUT)
HSRLE_DEF_PAIR(rle8_7symlut, HSRLE_RLE8_7SYMLUT)
HSRLE_DEF_WIDTH(16)
HSRLE_DEF_WIDTH(24)
HSRLE_DEF_WIDTH(32)
HSRLE_DEF_WIDTH(48)
HSRLE_DEF_WIDTH(64)
HSRLE_DEF_PAIR(rle128_sym, HSRLE_RLE128_SYM)
HSRLE_DEF_PAIR(rle128_sym_packed, HSRLE_RLE128_SYM_PACKED)
HSRLE_DEF_PAIR(rle128_byte, HSRLE_RLE128_BYTE)
HSRLE_DEF_PAIR(rle128_byte_packed, HSRLE_RLE128_BYTE_PACKED)
// Short family
#define HSRLE_DEF_SHORT_WIDTH(W)                                                                                                                            \
  HSRLE_DEF_PAIR(rle##W##_sym_short, codec_id(SHORT0, W / 8, 1)) HSRLE_DEF_PAIR(rle##W##_1symlut_sym_short, codec_id(SHORT1, W / 8, 1))                       \
  HSRLE_DEF_PAIR(rle##W##_3symlut_sym_short, codec_id(SHORT3, W / 8, 1)) HSRLE_DEF_PAIR(rle##W##_7symlut_sym_short, codec_id(SHORT7, W / 8, 1))               \
  HSRLE_DEF_PAIR(rle##W##_byte_short, codec_id(SHORT0, W / 8, 0)) HSRLE_DEF_PAIR(rle##W##_1symlut_byte_short, codec_id(SHORT1, W / 8, 0))                     \
  HSRLE_DEF_PAIR(rle##W##_3symlut_byte_short, codec_id(SHORT3, W / 8, 0)) HSRLE_DEF_PAIR(rle##W##_7symlut_byte_short, codec_id(SHORT7, W / 8, 0))
HSRLE_DEF_PAIR(rle8_multi_short, HSRLE_RLE8_MULTI_SHORT)
HSRLE_DEF_PAIR(rle8_1symlut_short, HSRLE_RLE8_1SYMLUT_SHORT)
HSRLE_DEF_PAIR(rle8_3symlut_short, HSRLE_RLE8_3SYMLUT_SHORT)
HSRLE_DEF_PAIR(rle8_7symlut_short, HSRLE_RLE8_7SYMLUT_SHORT)
HSRLE_DEF_SHORT_WIDTH(16)
HSRLE_DEF_SHORT_WIDTH(24)
HSRLE_DEF_SHORT_WIDTH(32)
HSRLE_DEF_SHORT_WIDTH(48)
HSRLE_DEF_SHORT_WIDTH(64)
// Greedy encoders: only a compress entry point each (src/rle.h:398-416); their streams go to rle{W}_{K}symlut_byte_short_decompress
#define HSRLE_DEF_GREEDY(W)                                                                                                                                           \
  uint32_t rle##W##_1symlut_byte_short_compress_greedy(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mono_compress(codec_id(SHORT1, W / 8, 0, true), pIn, inSize, pOut, outSize); } \
  uint32_t rle##W##_3symlut_byte_short_compress_greedy(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mono_compress(codec_id(SHORT3, W / 8, 0, true), pIn, inSize, pOut, outSize); } \
  uint32_t rle##W##_7symlut_byte_short_compress_greedy(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize) { return mono_compress(codec_id(SHORT7, W / 8, 0, true), pIn, inSize, pOut, outSize); }
HSRLE_DEF_GREEDY(16)
HSRLE_DEF_GREEDY(24)
HSRLE_DEF_GREEDY(32)
HSRLE_DEF_GREEDY(48)
HSRLE_DEF_GREEDY(64)
HSRLE_DEF_PAIR(rle8_single_short, HSRLE_RLE8_SINGLE_SHORT)

// ---- container API ----

uint64_t hsrle_container_bound(uint64_t inSize, uint32_t blockSize)
{
  if (blockSize == 0) blockSize = HSRLE_DEFAULT_BLOCK_SIZE;
  if (!valid_block_size(blockSize) || inSize == 0) return 0;
  const uint64_t nb = block_count(inSize, blockSize);
  return HSRLE_CONTAINER_HEADER_SIZE + 8ull * (nb + 1) + nb * (uint64_t)slot_stride(blockSize) + HSRLE_CONTAINER_TAIL_PAD;
}

uint64_t hsrle_compress_workspace_size(uint64_t inSize, uint32_t blockSize)
{
  if (blockSize == 0) blockSize = HSRLE_DEFAULT_BLOCK_SIZE;
  if (!valid_block_size(blockSize) || inSize == 0) return 0;
  return plan_workspace(inSize, blockSize).total;
}

uint64_t hsrle_compress_workspace_size_codec(int codec, uint64_t inSize, uint32_t blockSize)
{
  if (blockSize == 0) blockSize = HSRLE_DEFAULT_BLOCK_SIZE;
  if (!valid_block_size(blockSize) || inSize == 0 || codec < 0 || codec >= kCodecCount) return 0;
  // what the path of a workspace with every region needs: the small-block regions only where the split encode takes the container (the Greedy codecs with a
  // one-symbol list; round 6 made 8 bit Single and 128 bit position-parallel there), none where the windowed encoders do (1.05 x the input instead of 3.4 x)
  return plan_workspace(inSize, blockSize, encode_choice_of(codec, inSize, blockSize, SPLIT_ALL).regions).total;
}

int hsrle_compress_dev_async(int codec, const void *dIn, uint64_t inSize, void *dOut, uint64_t outCapacity, uint32_t blockSize, void *dWorkspace,
                             uint64_t workspaceSize, void *stream)
{
  return compress_async(codec, dIn, inSize, dOut, outCapacity, blockSize, dWorkspace, workspaceSize, (hipStream_t)stream);
}

int hsrle_compress_dev(int codec, const void *dIn, uint64_t inSize, void *dOut, uint64_t outCapacity, uint32_t blockSize, uint64_t *pContainerSize, void *stream)
{
  int rc = compress_async(codec, dIn, inSize, dOut, outCapacity, blockSize, nullptr, 0, (hipStream_t)stream);
  if (rc != HSRLE_OK) return rc;
  ContainerHeader h;
  if (hipMemcpyAsync(&h, dOut, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  static const char magic[8] = { 'H', 'S', 'R', 'L', 'E', 'K', 'I', 'T' };
  if (memcmp(h.magic, magic, 8) != 0)
  {
    // the split encode struck its own container (a per-lane chunk encoder missed its boundary run: k_split_verdict): the synchronous entry sees it here
    // and encodes the container again with one lane per block -- as the monolithic path falls back; the enqueue-only entry cannot
    rc = compress_async(codec, dIn, inSize, dOut, outCapacity, blockSize, nullptr, 0, (hipStream_t)stream, true);
    if (rc != HSRLE_OK) return rc;
    if (hipMemcpyAsync(&h, dOut, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
      return HSRLE_ERR_DEVICE;
    if (memcmp(h.magic, magic, 8) != 0) return HSRLE_ERR_DEVICE;
  }
  if (pContainerSize) *pContainerSize = h.totalSize;
  return HSRLE_OK;
}

int hsrle_container_info_host(const void *pContainer, uint64_t containerSize, hsrle_container_info_t *pInfo)
{
  if (!pContainer || !pInfo || containerSize < HSRLE_CONTAINER_HEADER_SIZE) return HSRLE_ERR_ARGUMENT;
  ContainerHeader h;
  memcpy(&h, pContainer, sizeof(h));
  return check_info(h, containerSize, pInfo);
}

int hsrle_container_info_dev(const void *dContainer, uint64_t containerSize, hsrle_container_info_t *pInfo, void *stream)
{
  if (!dContainer || !pInfo || containerSize < HSRLE_CONTAINER_HEADER_SIZE) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  ContainerHeader h;
  if (hipMemcpyAsync(&h, dContainer, sizeof(h), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  return check_info(h, containerSize, pInfo);
}

int hsrle_decompress_blocks_dev_async(const void *dContainer, const hsrle_container_info_t *info, uint32_t firstBlock, uint32_t blockCount, void *dOut,
                                      uint64_t outCapacity, uint32_t *dStatus, void *stream)
{
  return decompress_blocks_async(dContainer, info, firstBlock, blockCount, dOut, outCapacity, dStatus, (hipStream_t)stream);
}

int hsrle_decompress_dev_async(const void *dContainer, const hsrle_container_info_t *info, void *dOut, uint64_t outCapacity, uint32_t *dStatus, void *stream)
{
  if (!info) return HSRLE_ERR_ARGUMENT;
  return decompress_blocks_async(dContainer, info, 0, info->blockCount, dOut, outCapacity, dStatus, (hipStream_t)stream);
}

uint32_t hsrle_split_sub_block_size(const hsrle_container_info_t *info, uint32_t subBlockSize)
{
  if (!info || !valid_block_size(info->blockSize)) return 0;
  return split_sub_block(info, subBlockSize);
}

uint64_t hsrle_decompress_split_workspace_size(const hsrle_container_info_t *info, uint32_t blockCount, uint32_t subBlockSize)
{
  if (!info || !valid_block_size(info->blockSize)) return 0;
  const uint32_t SB = split_sub_block(info, subBlockSize);
  if (SB == info->blockSize) return 0;
  if (SB == HSRLE_SPLIT_PACKET_LIST) return packet_list_counts_bytes(blockCount) + (uint64_t)blockCount * packet_list_cap(info->blockSize) * 8ull;
  return (uint64_t)blockCount * (info->blockSize / SB) * 4ull * kEntryRecDwords;
}

int hsrle_decompress_split_dev_async(const void *dContainer, const hsrle_container_info_t *info, uint32_t firstBlock, uint32_t blockCount, void *dOut, uint64_t outCapacity,
                                     uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize, uint32_t subBlockSize, void *stream)
{
  return decompress_split_async(dContainer, info, firstBlock, blockCount, dOut, outCapacity, dStatus, dWorkspace, workspaceSize, subBlockSize, (hipStream_t)stream);
}

#ifdef HSRLE_EXPERIMENTS   // the wave-per-block decoder exists in experiment builds only (csrc/experiments/hsrle_decode_wave.hip.h)
int hsrle_decompress_wave_dev_async(const void *dContainer, const hsrle_container_info_t *info, uint32_t firstBlock, uint32_t blockCount, void *dOut, uint64_t outCapacity,
                                    uint32_t *dStatus, void *stream)
{
  return decompress_wave_async(dContainer, info, firstBlock, blockCount, dOut, outCapacity, dStatus, (hipStream_t)stream);
}
#endif

int hsrle_decompress_dev(const void *dContainer, uint64_t containerSize, void *dOut, uint64_t outCapacity, uint64_t *pUncompressedSize, void *stream)
{
  hsrle_container_info_t info;
  int rc = hsrle_container_info_dev(dContainer, containerSize, &info, stream);
  if (rc != HSRLE_OK) return rc;

  // a container with too few blocks to fill the GPU with one lane per block is decoded split (one lane per sub-block):
  // this call owns its scratch, so it can afford the records
  // ... or, for blocks of up to 16 KiB, by one WAVE per block (experiments/hsrle_decode_wave.hip.h): no records, no second kernel
  // (opt-in: measured on the 88 MB frame it is the slower of the two -- 427 us against 189 us split: the packet hops of ONE lane per
  //  wave are a latency chain of ~1 us per packet that the other 63 lanes wait for, while the split decode's record walk runs 64 such
  //  chains per wave)
  static const int waveMode = kExperiments ? (int)knob_u32("HSRLE_WAVE_DECODE", 0) : 0;
  const bool wave = waveMode != 0 && info.blockCount < kWaveDecodeBelow && info.blockSize <= 16384u && info.codec < (uint32_t)kCodecCount;
  const uint64_t recBytes = (!wave && info.blockCount < 131072u) ? hsrle_decompress_split_workspace_size(&info, info.blockCount, 0) : 0;
  uint8_t *scratch = (uint8_t *)scratch_alloc(256 + recBytes, (hipStream_t)stream);
  uint32_t *dStatus = (uint32_t *)scratch;
  if (!dStatus) return HSRLE_ERR_DEVICE;
  uint32_t status = 0;
  bool ok = hipMemsetAsync(dStatus, 0, 4, (hipStream_t)stream) == hipSuccess;
  if (ok)
  {
    if (wave)
      rc = decompress_wave_async(dContainer, &info, 0, info.blockCount, dOut, outCapacity, dStatus, (hipStream_t)stream);
    else if (recBytes != 0)
      rc = decompress_split_async(dContainer, &info, 0, info.blockCount, dOut, outCapacity, dStatus, scratch + 256, recBytes, 0, (hipStream_t)stream);
    else
      rc = decompress_blocks_async(dContainer, &info, 0, info.blockCount, dOut, outCapacity, dStatus, (hipStream_t)stream);
    ok = hipMemcpyAsync(&status, dStatus, 4, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess && hipStreamSynchronize((hipStream_t)stream) == hipSuccess;
  }
  scratch_free(dStatus, (hipStream_t)stream);
  if (rc != HSRLE_OK) return rc;
  if (!ok) return HSRLE_ERR_DEVICE;
  if (status != 0) return HSRLE_ERR_FORMAT;
  if (pUncompressedSize) *pUncompressedSize = info.uncompressedSize;
  return HSRLE_OK;
}

int hsrle_compress_host(int codec, const void *pIn, uint64_t inSize, void *pOut, uint64_t outCapacity, uint32_t blockSize, uint64_t *pContainerSize)
{
  if (!pIn || !pOut || inSize == 0) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  const uint64_t bound = hsrle_container_bound(inSize, blockSize);
  if (bound == 0) return HSRLE_ERR_ARGUMENT;

  void *dIn = nullptr, *dOut = nullptr;
  int rc = HSRLE_ERR_DEVICE;
  uint64_t total = 0;
  if (hipMalloc(&dIn, inSize) == hipSuccess && hipMalloc(&dOut, bound) == hipSuccess && hipMemcpy(dIn, pIn, inSize, hipMemcpyHostToDevice) == hipSuccess)
  {
    rc = hsrle_compress_dev(codec, dIn, inSize, dOut, bound, blockSize, &total, nullptr);
    if (rc == HSRLE_OK)
    {
      if (total > outCapacity) rc = HSRLE_ERR_CAPACITY;
      else if (hipMemcpy(pOut, dOut, total, hipMemcpyDeviceToHost) != hipSuccess) rc = HSRLE_ERR_DEVICE;
    }
  }
  if (dIn) (void)hipFree(dIn);
  if (dOut) (void)hipFree(dOut);
  if (rc == HSRLE_OK && pContainerSize) *pContainerSize = total;
  return rc;
}

int hsrle_decompress_host(const void *pContainer, uint64_t containerSize, void *pOut, uint64_t outCapacity, uint64_t *pUncompressedSize)
{
  hsrle_container_info_t info;
  int rc = hsrle_container_info_host(pContainer, containerSize, &info);
  if (rc != HSRLE_OK) return rc;
  if (!pOut || outCapacity < info.uncompressedSize) return HSRLE_ERR_CAPACITY;
  if (!device_ok()) return HSRLE_ERR_DEVICE;

  void *dIn = nullptr, *dOut = nullptr;
  rc = HSRLE_ERR_DEVICE;
  if (hipMalloc(&dIn, info.totalSize) == hipSuccess && hipMalloc(&dOut, info.uncompressedSize) == hipSuccess &&
      hipMemcpy(dIn, pContainer, info.totalSize, hipMemcpyHostToDevice) == hipSuccess)
  {
    uint64_t U = 0;
    rc = hsrle_decompress_dev(dIn, info.totalSize, dOut, info.uncompressedSize, &U, nullptr);
    if (rc == HSRLE_OK && hipMemcpy(pOut, dOut, U, hipMemcpyDeviceToHost) != hipSuccess) rc = HSRLE_ERR_DEVICE;
    if (rc == HSRLE_OK && pUncompressedSize) *pUncompressedSize = U;
  }
  if (dIn) (void)hipFree(dIn);
  if (dOut) (void)hipFree(dOut);
  return rc;
}

void hsrle_mono_tuning(uint32_t blockSize, uint32_t regionSize, uint32_t lookBack)
{
  g_monoTune[0] = blockSize; g_monoTune[1] = regionSize; g_monoTune[2] = lookBack;
}

void hsrle_mono_encode_stats(uint32_t stats[4])
{
  for (int k = 0; k < 4; k++) stats[k] = g_monoEncLast[k];
}

uint64_t hsrle_compress_mono_workspace_size(int codec, uint32_t inSize)
{
  if (codec < 0 || codec >= kCodecCount || inSize == 0 || inSize > (1u << 30)) return 0;
  return plan_mono_encode(inSize, codec).total;
}

int hsrle_compress_mono_dev(int codec, const void *dIn, uint32_t inSize, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize, uint32_t *pStreamSize,
                            uint32_t *pChunks, void *stream)
{
  if (!dIn || !dOut || !dWorkspace || !pStreamSize || codec < 0 || codec >= kCodecCount || inSize == 0) return HSRLE_ERR_ARGUMENT;
  if (inSize > (1u << 30)) return HSRLE_ERR_UNSUPPORTED;
  if (outCapacity < bounds32(inSize)) return HSRLE_ERR_CAPACITY;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  const MonoEncPlan m = plan_mono_encode(inSize, codec);
  if (workspaceSize < m.total) return HSRLE_ERR_CAPACITY;
  return mono_encode_dev(codec, (const uint8_t *)dIn, inSize, (uint8_t *)dOut, (uint8_t *)dWorkspace, m, pStreamSize, pChunks, (hipStream_t)stream);
}

int hsrle_compress_mono_dev_async(int codec, const void *dIn, uint32_t inSize, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize, uint32_t *dStreamSize,
                                  void *stream)
{
  if (!dIn || !dOut || !dWorkspace || codec < 0 || codec >= kCodecCount || inSize == 0) return HSRLE_ERR_ARGUMENT;
  if (inSize > (1u << 30)) return HSRLE_ERR_UNSUPPORTED;
  if (outCapacity < bounds32(inSize)) return HSRLE_ERR_CAPACITY;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  const MonoEncPlan m = plan_mono_encode(inSize, codec);
  if (!g_launch[codec].ppw8 || !m.windowed) return HSRLE_ERR_UNSUPPORTED;         // (the 8 bit pair only, as ever: the other codecs take hsrle_compress_mono_dev_enqueue)
  if (workspaceSize < m.total) return HSRLE_ERR_CAPACITY;
  return mono_encode_dev(codec, (const uint8_t *)dIn, inSize, (uint8_t *)dOut, (uint8_t *)dWorkspace, m, nullptr, dStreamSize, (hipStream_t)stream);
}

int hsrle_compress_mono_dev_enqueue(int codec, const void *dIn, uint32_t inSize, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize,
                                    uint32_t *dStreamSize, uint32_t *dStatus, void *stream)
{
  if (codec < 0 || codec >= kCodecCount) return HSRLE_ERR_ARGUMENT;
  if (!chunk_mode(kCodecs[codec])) return HSRLE_ERR_UNSUPPORTED;         // (before the device: the codec set is a property of the library)
  if (!dIn || !dOut || !dWorkspace || !dStatus || inSize == 0) return HSRLE_ERR_ARGUMENT;
  if (inSize > (1u << 30)) return HSRLE_ERR_UNSUPPORTED;
  if (outCapacity < bounds32(inSize)) return HSRLE_ERR_CAPACITY;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  const MonoEncPlan m = plan_mono_encode(inSize, codec);
  if (!m.windowed) return HSRLE_ERR_UNSUPPORTED;                          // (experiment builds that force the old flow)
  if (workspaceSize < m.total) return HSRLE_ERR_CAPACITY;
  return mono_encode_dev(codec, (const uint8_t *)dIn, inSize, (uint8_t *)dOut, (uint8_t *)dWorkspace, m, nullptr, dStreamSize, (hipStream_t)stream, dStatus);
}

uint64_t hsrle_decompress_mono_workspace_size(int codec, uint32_t uncompressedSize, uint32_t compressedSize)
{
  if (codec < 0 || codec >= kCodecCount || uncompressedSize == 0 || compressedSize < 10u) return 0;
  return plan_mono(codec, uncompressedSize, compressedSize, header_size(kCodecs[codec])).total + 16u;   // (+ 16: a workspace that is not 16-byte aligned is aligned here)
}

// the workspace is cleared with 16-byte stores (mono_prepare): a caller that sub-allocates from a byte pool may hand over any address -- it is rounded up, what
// is left must still hold the plan (hsrle_decompress_mono_workspace_size() includes the 16 bytes)
static inline void mono_align_workspace(void *&dWorkspace, uint64_t &workspaceSize)
{
  const uint64_t skip = (16u - (uint32_t)((uintptr_t)dWorkspace & 15u)) & 15u;
  dWorkspace = (uint8_t *)dWorkspace + skip;
  workspaceSize = workspaceSize > skip ? workspaceSize - skip : 0u;
}

int hsrle_decompress_mono_dev(int codec, const void *dStream, uint32_t streamSize, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize,
                              uint32_t *pUncompressedSize, uint32_t *pStats, void *stream)
{
  if (!dStream || !dOut || !dWorkspace || codec < 0 || codec >= kCodecCount || streamSize < header_size(kCodecs[codec]) || ((uintptr_t)dStream & 127u) != 0u)
    return HSRLE_ERR_ARGUMENT;
  mono_align_workspace(dWorkspace, workspaceSize);
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  uint8_t h16[16] = { 0 };
  if (hipMemcpyAsync(h16, dStream, streamSize < 16u ? streamSize : 16u, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  MonoHeader mh;
  if (!mono_header(codec, h16, streamSize, clamp32(outCapacity), &mh))
    return HSRLE_ERR_FORMAT;
  const MonoPlan m = plan_mono(mh.codec, mh.U, mh.C, mh.p0);
  if (workspaceSize < m.total) return HSRLE_ERR_CAPACITY;
  const int rc = mono_decode_dev(mh, (const uint8_t *)dStream, (uint8_t *)dOut, (uint8_t *)dWorkspace, m, pStats, (hipStream_t)stream);
  if (rc == HSRLE_OK && pUncompressedSize) *pUncompressedSize = mh.U;
  return rc;
}

int hsrle_decompress_mono_dev_async(int codec, const void *dStream, const uint8_t *pHeader16, uint32_t streamSize, void *dOut, uint64_t outCapacity, void *dWorkspace,
                                    uint64_t workspaceSize, uint32_t *pUncompressedSize, uint32_t *dStatus, void *stream)
{
  // (the same smallest stream as the synchronous entry: the codec's header; pHeader16 holds the stream's first min(16, streamSize) bytes, zeros behind them)
  if (!dStream || !pHeader16 || !dOut || !dWorkspace || !dStatus || codec < 0 || codec >= kCodecCount || streamSize < header_size(kCodecs[codec]) || ((uintptr_t)dStream & 127u) != 0u)
    return HSRLE_ERR_ARGUMENT;
  mono_align_workspace(dWorkspace, workspaceSize);
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  MonoHeader mh;
  if (!mono_header(codec, pHeader16, streamSize, clamp32(outCapacity), &mh))
    return HSRLE_ERR_FORMAT;
  const MonoPlan m = plan_mono(mh.codec, mh.U, mh.C, mh.p0);
  if (workspaceSize < m.total) return HSRLE_ERR_CAPACITY;
  MonoRun run;
  int rc = mono_prepare(mh, (const uint8_t *)dStream, (uint8_t *)dOut, (uint8_t *)dWorkspace, m, &run, (hipStream_t)stream);
  if (rc == HSRLE_OK) rc = mono_enqueue_first_try(mh, (uint8_t *)dWorkspace, m, run, (hipStream_t)stream);
  if (rc != HSRLE_OK) return rc;
  hipLaunchKernelGGL(k_mono_status, dim3(1), dim3(1), 0, (hipStream_t)stream, (const uint32_t *)run.ctrl, dStatus);
  if (hipGetLastError() != hipSuccess) return HSRLE_ERR_DEVICE;
  if (pUncompressedSize) *pUncompressedSize = mh.U;
  return HSRLE_OK;
}

uint64_t hsrle_mono_index_size(int codec, uint32_t uncompressedSize, uint32_t compressedSize, uint32_t spacing)
{
  if (codec < 0 || codec >= kCodecCount || uncompressedSize == 0 || compressedSize < 10u || (spacing != 0u && !valid_spacing(spacing))) return 0;
  const MonoPlan m = plan_mono(codec, uncompressedSize, compressedSize, header_size(kCodecs[codec]), spacing);
  return kMonoIndexHeaderBytes + m.nb * kMonoIndexRecordBytes;
}

uint64_t hsrle_mono_index_workspace_size(int codec, uint32_t uncompressedSize, uint32_t compressedSize, uint32_t spacing)
{
  if (codec < 0 || codec >= kCodecCount || uncompressedSize == 0 || compressedSize < 10u || (spacing != 0u && !valid_spacing(spacing))) return 0;
  return plan_mono(codec, uncompressedSize, compressedSize, header_size(kCodecs[codec]), spacing).total + 16u;   // (+ 16: as hsrle_decompress_mono_workspace_size)
}

int hsrle_mono_index_build_dev(int codec, const void *dStream, uint32_t streamSize, uint32_t spacing, void *dIndex, uint64_t indexCapacity, void *dWorkspace,
                               uint64_t workspaceSize, hsrle_mono_index_info_t *pInfo, void *stream)
{
  if (!dStream || !dIndex || !dWorkspace || codec < 0 || codec >= kCodecCount || streamSize < header_size(kCodecs[codec]) || ((uintptr_t)dStream & 127u) != 0u ||
      ((uintptr_t)dIndex & 15u) != 0u || (spacing != 0u && !valid_spacing(spacing)))
    return HSRLE_ERR_ARGUMENT;
  mono_align_workspace(dWorkspace, workspaceSize);
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  const hipStream_t st = (hipStream_t)stream;
  uint8_t h16[16] = { 0 };
  if (hipMemcpyAsync(h16, dStream, streamSize < 16u ? streamSize : 16u, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  MonoHeader mh;
  if (!mono_header(codec, h16, streamSize, 0xFFFFFFFFu, &mh))
    return HSRLE_ERR_FORMAT;
  const MonoPlan m = plan_mono(mh.codec, mh.U, mh.C, mh.p0, spacing);
  if (workspaceSize < m.total) return HSRLE_ERR_CAPACITY;
  const uint64_t indexBytes = kMonoIndexHeaderBytes + m.nb * kMonoIndexRecordBytes;
  if (indexCapacity < indexBytes) return HSRLE_ERR_CAPACITY;
  uint32_t *const rec = (uint32_t *)((uint8_t *)dIndex + kMonoIndexHeaderBytes);
  // the walk, the proof, the repairs and the records pass of the monolithic decode, the records written behind the header; then the tags
  int rc = mono_decode_dev(mh, (const uint8_t *)dStream, nullptr, (uint8_t *)dWorkspace, m, nullptr, st, rec);
  if (rc != HSRLE_OK) return rc;
  hipLaunchKernelGGL(k_index_tags, dim3((uint32_t)((m.nb + 255u) / 256u)), dim3(256), 0, st, (const uint8_t *)dStream, mh.C, rec, (uint32_t)m.nb);
  if (hipGetLastError() != hipSuccess) return HSRLE_ERR_DEVICE;
  MonoIndexHeader h;
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, kMonoIndexMagic, 8);
  h.version = kMonoIndexVersion; h.codec = (uint32_t)codec; h.U = mh.U; h.C = mh.C; h.spacing = m.B; h.recordCount = (uint32_t)m.nb; h.recordBytes = kMonoIndexRecordBytes;
  for (uint32_t j = 0; j < 16u && j < mh.C; j++) h.head[j] = h16[j];
  h.indexBytes = indexBytes;
  if (hipMemcpyAsync(dIndex, &h, sizeof(h), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
    return HSRLE_ERR_DEVICE;
  if (pInfo) rc = hsrle_mono_index_info_host(&h, sizeof(h) + m.nb * kMonoIndexRecordBytes, pInfo);
  return rc;
}

int hsrle_mono_index_info_host(const void *pIndex, uint64_t size, hsrle_mono_index_info_t *pInfo)
{
  if (!pIndex || !pInfo) return HSRLE_ERR_ARGUMENT;
  if (size < kMonoIndexHeaderBytes) return HSRLE_ERR_FORMAT;
  MonoIndexHeader h;
  memcpy(&h, pIndex, sizeof(h));
  hsrle_mono_index_info_t info;
  info.version = h.version; info.codec = h.codec; info.uncompressedSize = h.U; info.compressedSize = h.C;
  info.spacing = h.spacing; info.recordCount = h.recordCount; info.recordBytes = h.recordBytes;
  memcpy(info.streamHead, h.head, 16);
  info.indexBytes = h.indexBytes;
  MonoHeader mh;
  if (memcmp(h.magic, kMonoIndexMagic, 8) != 0 || h.reserved != 0u || !mono_index_info_ok(&info, &mh) || size < info.indexBytes)
    return HSRLE_ERR_FORMAT;
  *pInfo = info;
  return HSRLE_OK;
}

int hsrle_mono_decompress_range_dev_async(const void *dStream, const void *dIndex, const hsrle_mono_index_info_t *info, uint64_t offset, uint64_t length, void *dOut,
                                          uint64_t outCapacity, uint32_t *dStatus, void *stream)
{
  if (!dStream || !dIndex || !info || !dOut || !dStatus || ((uintptr_t)dStream & 127u) != 0u || ((uintptr_t)dIndex & 15u) != 0u)
    return HSRLE_ERR_ARGUMENT;
  MonoHeader mh;
  if (!mono_index_info_ok(info, &mh))
    return HSRLE_ERR_FORMAT;
  if (offset > info->uncompressedSize || length > info->uncompressedSize - offset || outCapacity < length)
    return HSRLE_ERR_ARGUMENT;
  if (length == 0u)
    return HSRLE_OK;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  init_tables();
  if (!g_launch[mh.codec].dec)
    return HSRLE_ERR_UNSUPPORTED;
  const hipStream_t st = (hipStream_t)stream;
  const uint32_t B = info->spacing, first = (uint32_t)(offset / B), n = (uint32_t)((offset + length - 1u) / B) - first + 1u;
  const uint32_t *rec = (const uint32_t *)((const uint8_t *)dIndex + kMonoIndexHeaderBytes);
  u32x4 head;
  memcpy(&head, info->streamHead, 16);
  hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, st, dStatus, 0u);
  hipLaunchKernelGGL(k_range_gate, dim3((n + 255u) / 256u), dim3(256), 0, st, (const uint8_t *)dStream, mh.C, head, rec, first, n, dStatus);
  if (hipGetLastError() != hipSuccess) return HSRLE_ERR_DEVICE;
  // lanes first .. first + n - 1, each from its record; only [offset, offset + length) is stored, at dOut.  The status word is the gate: a mismatch
  // stops every workgroup (a decode error seen by an early workgroup may stop later ones too -- the result is MALFORMED either way)
  DecodeArgs da{ (const uint8_t *)dStream, nullptr, (const uint8_t *)dStream + mh.C + HSRLE_CONTAINER_TAIL_PAD, (uint8_t *)dOut, mh.U, B, first, n, dStatus };
  da.entries = rec; da.entryBase = 0; da.gate = dStatus; da.gateWords = 1; da.winLo = offset; da.winHi = offset + length;
  if (g_launch[mh.codec].dec(da, st) != hipSuccess) return HSRLE_ERR_DEVICE;
  hipLaunchKernelGGL(k_range_status, dim3(1), dim3(1), 0, st, dStatus);
  return hipGetLastError() == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

int hsrle_decompress_range_dev_async(const void *dContainer, const hsrle_container_info_t *info, uint64_t offset, uint64_t length, void *dOut, uint64_t outCapacity,
                                     uint32_t *dStatus, void *stream)
{
  if (!dContainer || !info || !dOut || !dStatus)
    return HSRLE_ERR_ARGUMENT;
  if (info->codec >= (uint32_t)kCodecCount || !valid_block_size(info->blockSize) || info->blockCount != block_count(info->uncompressedSize, info->blockSize))
    return HSRLE_ERR_FORMAT;
  if (offset > info->uncompressedSize || length > info->uncompressedSize - offset || outCapacity < length)
    return HSRLE_ERR_ARGUMENT;
  if (length == 0u)
    return HSRLE_OK;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  init_tables();
  if (!g_launch[info->codec].dec)
    return HSRLE_ERR_UNSUPPORTED;
  const hipStream_t st = (hipStream_t)stream;
  const uint32_t first = (uint32_t)(offset / info->blockSize), n = (uint32_t)((offset + length - 1u) / info->blockSize) - first + 1u;
  const uint8_t *container = (const uint8_t *)dContainer;
  const uint8_t *payload = container + HSRLE_CONTAINER_HEADER_SIZE + 8ull * ((uint64_t)info->blockCount + 1ull);
  hipLaunchKernelGGL(k_set_word, dim3(1), dim3(1), 0, st, dStatus, 0u);
  DecodeArgs da{ payload, (const uint64_t *)(container + HSRLE_CONTAINER_HEADER_SIZE), payload + info->payloadSize + HSRLE_CONTAINER_TAIL_PAD,
                 (uint8_t *)dOut, info->uncompressedSize, info->blockSize, first, n, dStatus };
  da.winLo = offset; da.winHi = offset + length;
  if (g_launch[info->codec].dec(da, st) != hipSuccess) return HSRLE_ERR_DEVICE;
  hipLaunchKernelGGL(k_range_status, dim3(1), dim3(1), 0, st, dStatus);
  return hipGetLastError() == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

int hsrle_hash_blocks_dev_async(const void *dContainer, const hsrle_container_info_t *info, uint32_t firstBlock, uint32_t blockCount, uint64_t *dHashes, void *stream)
{
  if (!dContainer || !info || !dHashes || (uint64_t)firstBlock + blockCount > info->blockCount) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  if (blockCount == 0) return HSRLE_OK;
  const uint8_t *container = (const uint8_t *)dContainer;
  const uint8_t *payload = container + HSRLE_CONTAINER_HEADER_SIZE + 8ull * ((uint64_t)info->blockCount + 1ull);
  hipLaunchKernelGGL(k_hash_blocks, dim3((blockCount + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, payload, (const uint64_t *)(container + HSRLE_CONTAINER_HEADER_SIZE),
                     info->payloadSize, firstBlock, blockCount, dHashes);
  return hipGetLastError() == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

int hsrle_synth_dev_async(int kind, int symbolBytes, uint64_t seed, void *dOut, uint64_t size, void *stream)
{
  if (!dOut || size == 0 || (kind != HSRLE_SYNTH_RUNS && kind != HSRLE_SYNTH_VIDEO) || symbolBytes < 1 || symbolBytes > 16) return HSRLE_ERR_ARGUMENT;
  if (!device_ok()) return HSRLE_ERR_DEVICE;
  const uint64_t chunks = (size + kSynthChunk - 1) / kSynthChunk;
  hipLaunchKernelGGL(k_synth, dim3((uint32_t)((chunks + 63) / 64)), dim3(64), 0, (hipStream_t)stream, kind, symbolBytes, seed, (uint8_t *)dOut, size);
  return hipGetLastError() == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

} // extern "C"
