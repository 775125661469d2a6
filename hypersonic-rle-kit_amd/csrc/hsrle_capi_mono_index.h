// hsrle_capi_mono_index.h -- part of hsrle_capi.hip: header, record tags and the range decode's gate of the
// persistent index of a monolithic stream (hsrle_mono_index_*): the proven entry records of mono_decode_dev, kept behind a 64-byte header
// in a buffer of the caller's, and the range decode that starts the block kernel's lanes from them.  Little endian, no pointers:
//   [ 0] char     magic[8] = "HSRLEIDX"     [ 8] uint32_t version = 1     [12] uint32_t codec
//   [16] uint32_t uncompressedSize           [20] uint32_t compressedSize  (both as in the stream's header)
//   [24] uint32_t spacing                    [28] uint32_t recordCount = ceil(uncompressedSize / spacing)
//   [32] uint32_t recordBytes = 96           [36] uint32_t reserved = 0
//   [40] uint8_t  streamHead[16]  (the stream's first min(16, compressedSize) bytes, zeros behind)
//   [56] uint64_t indexBytes = 64 + recordCount * recordBytes
//   [64] records: entry record k (hsrle_common.hip.h kEntryRecDwords) = the decoder state at output position k * spacing; its stream
//        position is relative to the stream's first byte, dwords a codec does not use are zero, and the high half of dword 4 holds
//        a 16-bit tag of the 16 stream bytes at that position (the decoder reads only the low half of that dword)
#pragma once
#include "hsrle_capi_mono_decode.h"

namespace hsrle {

constexpr uint32_t kMonoIndexVersion = 1u;
constexpr uint32_t kMonoIndexHeaderBytes = 64u;
constexpr uint32_t kMonoIndexRecordBytes = 4u * kEntryRecDwords;
constexpr uint32_t kRangeMismatch = 0x80000000u;    // range decode status word: the gate kernel's verdict (the decoder's error bits are the low ones)

struct MonoIndexHeader
{
  char magic[8];
  uint32_t version, codec, U, C, spacing, recordCount, recordBytes, reserved;
  uint8_t head[16];
  uint64_t indexBytes;
};
static_assert(sizeof(MonoIndexHeader) == kMonoIndexHeaderBytes, "index header is 64 bytes");
static const char kMonoIndexMagic[8] = { 'H', 'S', 'R', 'L', 'E', 'I', 'D', 'X' };

static bool valid_spacing(uint32_t spacing) { return spacing >= 128u && spacing <= (1u << 20) && (spacing % 128u) == 0u; }

// the info a range decode is handed (or a header that was read) against itself: sizes, spacing, record count, and the stream head's own header
static bool mono_index_info_ok(const hsrle_mono_index_info_t *info, MonoHeader *mh)
{
  if (info->version != kMonoIndexVersion || info->codec >= (uint32_t)kCodecCount || info->uncompressedSize == 0u || !valid_spacing(info->spacing))
    return false;
  const uint64_t n = ((uint64_t)info->uncompressedSize + info->spacing - 1u) / info->spacing;
  if (info->recordCount != n || info->recordBytes != kMonoIndexRecordBytes || info->indexBytes != kMonoIndexHeaderBytes + n * kMonoIndexRecordBytes)
    return false;
  return mono_header((int)info->codec, info->streamHead, info->compressedSize, info->uncompressedSize, mh) && mh->U == info->uncompressedSize && mh->C == info->compressedSize;
}

// 16-bit tag of the (at most 16) stream bytes at position pos: what ties a record to the stream it was built from
__device__ __forceinline__ uint32_t record_tag(const uint8_t *__restrict__ s, uint32_t C, uint32_t pos)
{
  uint32_t h = 0x811C9DC5u;
#pragma unroll
  for (uint32_t j = 0; j < 16u; j++)
    h = (h ^ ((pos + j < C) ? (uint32_t)s[pos + j] : 0u)) * 0x01000193u;
  return (h ^ (h >> 16)) & 0xFFFFu;
}

__global__ __launch_bounds__(256) void k_index_tags(const uint8_t *__restrict__ s, uint32_t C, uint32_t *__restrict__ rec, uint32_t n)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t *const r = rec + (uint64_t)i * kEntryRecDwords;
  r[4] = (r[4] & 0xFFFFu) | (record_tag(s, C, r[0]) << 16);
}

// range decode, in front of the block kernel: does the index belong to this stream?  Thread 0 compares the header's stream head with the
// stream's first bytes, every thread one record's tag with the stream bytes at its position.  A mismatch sets kRangeMismatch in the status
// word, which the block kernel takes as its gate (it then writes nothing).
__global__ __launch_bounds__(256) void k_range_gate(const uint8_t *__restrict__ s, uint32_t C, u32x4 head, const uint32_t *__restrict__ rec, uint32_t first, uint32_t n,
                                                    uint32_t *__restrict__ status)
{
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool bad = false;
  if (i == 0u)
#pragma unroll
    for (uint32_t j = 0; j < 16u; j++)
      bad |= ((j < C) ? (uint32_t)s[j] : 0u) != ((head[j >> 2] >> (8u * (j & 3u))) & 0xFFu);
  if (i < n)
  {
    const uint32_t *const r = rec + (uint64_t)(first + i) * kEntryRecDwords;
    const uint32_t pos = r[0];
    bad |= r[1] != 0u || pos >= C || r[5] != C - pos || (r[4] >> 16) != record_tag(s, C, pos);
  }
  if (bad) atomicOr(status, kRangeMismatch);
}

// the range decodes' one word for the caller
__global__ void k_range_status(uint32_t *status)
{
  const uint32_t v = *status;
  *status = (v & kRangeMismatch) != 0u ? (uint32_t)HSRLE_MONO_INDEX_MISMATCH : (v != 0u ? (uint32_t)HSRLE_MONO_MALFORMED : (uint32_t)HSRLE_MONO_DONE);
}

} // namespace hsrle
