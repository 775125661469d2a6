// 128 bit symbols: rle128_{sym,byte}[_packed]  (reference: src/rle.h:124-125, :146-147, :168-169, :194-195)
#include "hsrle_decode.hip.h"
#include "hsrle_encode.hip.h"
#include "hsrle_encode128.hip.h"
#include "hsrle_index.hip.h"
#include "hsrle_launch.h"

namespace hsrle {

static_assert(small_ring_per_mille(kCodecs[codec_id(PLAIN, 16, 1)]) == 0u, "the codec rows (hsrle_codecs.h) give this width a 64-byte ring: instantiate it");
static hipError_t dec_sym(const DecodeArgs &a, hipStream_t st) { return windowed(a) ? launch_decode(k_decode_blocks<PLAIN, 16, 1, kDecodeTile, kDecodeRing, kDecodeStep, true, true, true>, a, st) : a.entries ? launch_decode(k_decode_blocks<PLAIN, 16, 1, kDecodeTile, kDecodeRing, kDecodeStep>, a, st) : launch_decode(k_decode_blocks<PLAIN, 16, 1, kDecodeTile, kDecodeRing, kDecodeStep, true, false>, a, st); }
static hipError_t dec_sym_packed(const DecodeArgs &a, hipStream_t st) { return windowed(a) ? launch_decode(k_decode_blocks<PACKED, 16, 1, kDecodeTile, kDecodeRing, kDecodeStep, true, true, true>, a, st) : a.entries ? launch_decode(k_decode_blocks<PACKED, 16, 1, kDecodeTile, kDecodeRing, kDecodeStep>, a, st) : launch_decode(k_decode_blocks<PACKED, 16, 1, kDecodeTile, kDecodeRing, kDecodeStep, true, false>, a, st); }
static hipError_t dec_byte(const DecodeArgs &a, hipStream_t st) { return windowed(a) ? launch_decode(k_decode_blocks<PLAIN, 16, 0, kDecodeTile, kDecodeRing, kDecodeStep, true, true, true>, a, st) : a.entries ? launch_decode(k_decode_blocks<PLAIN, 16, 0, kDecodeTile, kDecodeRing, kDecodeStep>, a, st) : launch_decode(k_decode_blocks<PLAIN, 16, 0, kDecodeTile, kDecodeRing, kDecodeStep, true, false>, a, st); }
static hipError_t dec_byte_packed(const DecodeArgs &a, hipStream_t st) { return windowed(a) ? launch_decode(k_decode_blocks<PACKED, 16, 0, kDecodeTile, kDecodeRing, kDecodeStep, true, true, true>, a, st) : a.entries ? launch_decode(k_decode_blocks<PACKED, 16, 0, kDecodeTile, kDecodeRing, kDecodeStep>, a, st) : launch_decode(k_decode_blocks<PACKED, 16, 0, kDecodeTile, kDecodeRing, kDecodeStep, true, false>, a, st); }

// ring encoder (hsrle_encode128.hip.h) for block sizes up to 64 KiB; HSRLE_ENCODE128_V1=1 selects the first-generation kernel (A/B runs)
template <int FAM, int AL>
static hipError_t enc_any(const EncodeArgs &a, hipStream_t st)
{
  static const bool v1 = knob_u32("HSRLE_ENCODE128_V1", 0u) != 0u;
  if (v1 || a.B > 65536u) return launch_encode(k_encode_blocks<FAM, 16, AL>, a, st);   // (the one-block drop-in path spans the whole input with one block: one lane either way)
  return launch_encode(k_encode128_blocks<FAM == PACKED, AL>, a, st, 0);
}
static hipError_t enc_sym(const EncodeArgs &a, hipStream_t st) { return enc_any<PLAIN, 1>(a, st); }
static hipError_t enc_sym_packed(const EncodeArgs &a, hipStream_t st) { return enc_any<PACKED, 1>(a, st); }
static hipError_t enc_byte(const EncodeArgs &a, hipStream_t st) { return enc_any<PLAIN, 0>(a, st); }
static hipError_t enc_byte_packed(const EncodeArgs &a, hipStream_t st) { return enc_any<PACKED, 0>(a, st); }

static hipError_t idx_sym(const IndexArgs &a, int records, hipStream_t st) { return launch_index<PLAIN, 16, 1>(a, records, st); }
static hipError_t idx_sym_packed(const IndexArgs &a, int records, hipStream_t st) { return launch_index<PACKED, 16, 1>(a, records, st); }
static hipError_t idx_byte(const IndexArgs &a, int records, hipStream_t st) { return launch_index<PLAIN, 16, 0>(a, records, st); }
static hipError_t idx_byte_packed(const IndexArgs &a, int records, hipStream_t st) { return launch_index<PACKED, 16, 0>(a, records, st); }

static hipError_t sub_sym(const DecodeArgs &a, uint32_t SB, uint32_t *rec, hipStream_t st) { return launch_sub_or_wave<PLAIN, 16, 1>(a, SB, 0u, rec, st); }
static hipError_t sub_sym_packed(const DecodeArgs &a, uint32_t SB, uint32_t *rec, hipStream_t st) { return launch_sub_or_wave<PACKED, 16, 1>(a, SB, 0u, rec, st); }
static hipError_t sub_byte(const DecodeArgs &a, uint32_t SB, uint32_t *rec, hipStream_t st) { return launch_sub_or_wave<PLAIN, 16, 0>(a, SB, 0u, rec, st); }
static hipError_t sub_byte_packed(const DecodeArgs &a, uint32_t SB, uint32_t *rec, hipStream_t st) { return launch_sub_or_wave<PACKED, 16, 0>(a, SB, 0u, rec, st); }

// chunks of one monolithic stream (hsrle_mono_encode.hip.h): the first-generation encoder, one lane per chunk, from its place behind a stored run
template <int FAM, int AL>
static hipError_t menc_any(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st)
{
  hipLaunchKernelGGL((k_encode128_chunks<FAM, AL>), dim3((a.nBlocks + 63u) / 64u), dim3(64), 0, st, a.in, a.U, a.nBlocks, m.starts, m.syms, m.slotOff, a.slots, a.sizes, a.B, (const uint32_t *)a.ringSel);
  return hipGetLastError();
}

void register_w128(DecodeLaunch *dec, EncodeLaunch *enc, IndexLaunch *idx, SubBlockLaunch *sub, MonoEncodeLaunch *menc)
{
  constexpr int sym = codec_id(PLAIN, 16, 1), symPacked = codec_id(PACKED, 16, 1), byte = codec_id(PLAIN, 16, 0), bytePacked = codec_id(PACKED, 16, 0);
  menc[sym] = menc_any<PLAIN, 1>; menc[symPacked] = menc_any<PACKED, 1>; menc[byte] = menc_any<PLAIN, 0>; menc[bytePacked] = menc_any<PACKED, 0>;
  sub[sym] = sub_sym; sub[symPacked] = sub_sym_packed; sub[byte] = sub_byte; sub[bytePacked] = sub_byte_packed;
  idx[sym] = idx_sym; idx[symPacked] = idx_sym_packed; idx[byte] = idx_byte; idx[bytePacked] = idx_byte_packed;
  dec[sym] = dec_sym;               enc[sym] = enc_sym;
  dec[symPacked] = dec_sym_packed;  enc[symPacked] = enc_sym_packed;
  dec[byte] = dec_byte;             enc[byte] = enc_byte;
  dec[bytePacked] = dec_byte_packed; enc[bytePacked] = enc_byte_packed;
}

} // namespace hsrle
