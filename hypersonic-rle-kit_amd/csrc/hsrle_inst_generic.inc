// hsrle_inst_generic.inc -- instantiates the 8 codecs of one symbol width (16/24/32/48/64 bit).
// Included by inst_wNN.hip with HSRLE_W (bits) and HSRLE_S (bytes) defined.
#include "hsrle_decode.hip.h"
#include "hsrle_encode.hip.h"
#include "hsrle_encodeS.hip.h"
#include "hsrle_encode_greedy.hip.h"
#include "hsrle_index.hip.h"
#include "hsrle_launch.h"

namespace hsrle {

#define HSRLE_CAT2(a, b) a##b
#define HSRLE_CAT(a, b) HSRLE_CAT2(a, b)

// HSRLE_ENCODE_V1=1 selects the first-generation encoder (per-lane global reads and writes, hsrle_encode.hip.h) for A/B runs
#ifdef HSRLE_ENCODE_V1
#define HSRLE_ENCODE_KERNEL k_encode_blocks
#else
#define HSRLE_ENCODE_KERNEL k_encodeS_blocks
#endif

// 2 byte symbols: the decoder's stream ring is chosen by the container's ratio (launch_decode_ring, hsrle_launch.h)
#if HSRLE_S == 2
#define HSRLE_DECODE_LAUNCH(FAM, AL) (windowed(a) ? launch_decode(k_decode_blocks<FAM, 2, AL, kDecodeTile, kDecodeRing, kDecodeStep, true, true, true>, a, st) : (a.entries ? launch_decode(k_decode_blocks<FAM, 2, AL, kDecodeTile, kDecodeRing, kDecodeStep>, a, st) \
                                                : launch_decode_ring<codec_id(FAM, 2, AL)>(k_decode_blocks<FAM, 2, AL, kDecodeTile, kDecodeRing, kDecodeStep, true, false>, \
                                                                                            k_decode_blocks<FAM, 2, AL, kDecodeTile, 64, kDecodeStep, true, false>, a, st)))
#elif HSRLE_S >= 6 && !defined(HSRLE_DECODE_ALWAYS_ENT)
// 6 / 8 byte symbols: no small ring (their packets are large: below a ratio of 0.2 the 64-byte ring cost the 7-symbol LUT codecs 24 % on
// run-distributed data, 19 % on video-shaped; sweep of 8 GiB buffers); plain containers take the instantiation without the record prologue
static_assert(small_ring_per_mille(kCodecs[codec_id(PLAIN, HSRLE_S, 1)]) == 0u, "the codec rows (hsrle_codecs.h) give this width a 64-byte ring: instantiate it");
#define HSRLE_DECODE_LAUNCH(FAM, AL) (windowed(a) ? launch_decode(k_decode_blocks<FAM, HSRLE_S, AL, kDecodeTile, kDecodeRing, kDecodeStep, true, true, true>, a, st) : (a.entries ? launch_decode(k_decode_blocks<FAM, HSRLE_S, AL, kDecodeTile, kDecodeRing, kDecodeStep>, a, st) \
                                                : launch_decode(k_decode_blocks<FAM, HSRLE_S, AL, kDecodeTile, kDecodeRing, kDecodeStep, true, false>, a, st)))
#elif HSRLE_S >= 3 && !defined(HSRLE_DECODE_ALWAYS_ENT)
// plain containers take the instantiation without the entry-record prologue (hsrle_decode.hip.h: ENT; same-box A/B on run-distributed
// data: rle32_3symlut_byte +6 %, rle48_7symlut_sym +4 %, rle64_sym +-0; the 128 bit codecs +10 %)
#define HSRLE_DECODE_LAUNCH(FAM, AL) (windowed(a) ? launch_decode(k_decode_blocks<FAM, HSRLE_S, AL, kDecodeTile, kDecodeRing, kDecodeStep, true, true, true>, a, st) : (a.entries ? launch_decode(k_decode_blocks<FAM, HSRLE_S, AL, kDecodeTile, kDecodeRing, kDecodeStep>, a, st) \
                                                : launch_decode_ring<codec_id(FAM, HSRLE_S, AL)>(k_decode_blocks<FAM, HSRLE_S, AL, kDecodeTile, kDecodeRing, kDecodeStep, true, false>, \
                                                                                                  k_decode_blocks<FAM, HSRLE_S, AL, kDecodeTile, 64, kDecodeStep, true, false>, a, st)))
#else
#define HSRLE_DECODE_LAUNCH(FAM, AL) (windowed(a) ? launch_decode(k_decode_blocks<FAM, HSRLE_S, AL, kDecodeTile, kDecodeRing, kDecodeStep, true, true, true>, a, st) : launch_decode(k_decode_blocks<FAM, HSRLE_S, AL, kDecodeTile, kDecodeRing, kDecodeStep>, a, st))
#endif

// Round 6: every codec of 2 .. 8 byte symbols except Greedy is position-parallel for blocks up to 4 KiB (hsrle_capi.hip: pp_applies) -- the run list encoders of
// these widths (hsrle_encodeSr.hip.h: small containers of 1 .. 4 KiB blocks, and big containers of 3 / 4 byte symbols on run-distributed data) had nothing left to
// take and are gone.  What is launched here: blocks above 4 KiB.
// 2 byte symbols: the history ring is chosen per input (launch_encode_ring, hsrle_launch.h); wider ones always use 128 bytes
template <int FAM, int AL>
static hipError_t enc_ring_launch(const EncodeArgs &a, hipStream_t st)
{
#if HSRLE_S == 2 && !defined(HSRLE_ENCODE_V1) && !defined(HSRLE_ENCS_RING)
  return launch_encode_ring<2>(k_encodeS_blocks<FAM, 2, AL, false, 256>, k_encodeS_blocks<FAM, 2, AL, false, 128>, a, st);
#elif (HSRLE_S == 3 || HSRLE_S == 4) && !defined(HSRLE_ENCODE_V1) && !defined(HSRLE_ENCS_RING)
  return launch_encode(k_encodeS_blocks<FAM, HSRLE_S, AL>, a, st, 0);
#else
  return launch_encode(HSRLE_ENCODE_KERNEL<FAM, HSRLE_S, AL>, a, st, 0);
#endif
}
#define HSRLE_ENCODE_LAUNCH(FAM, AL) enc_ring_launch<FAM, AL>(a, st)
#define HSRLE_ENCODE_LAUNCH_RL(FAM, AL) enc_ring_launch<FAM, AL>(a, st)

#define HSRLE_DEF(FAM, AL, TAG)                                                                                                        \
  static hipError_t dec_##TAG(const DecodeArgs &a, hipStream_t st) { return HSRLE_DECODE_LAUNCH(FAM, AL); } \
  static hipError_t enc_##TAG(const EncodeArgs &a, hipStream_t st) { return HSRLE_ENCODE_LAUNCH(FAM, AL); } \
  static hipError_t idx_##TAG(const IndexArgs &a, int records, hipStream_t st) { return launch_index<FAM, HSRLE_S, AL>(a, records, st); } \
  static hipError_t sub_##TAG(const DecodeArgs &a, uint32_t SB, uint32_t *rec, hipStream_t st) { return launch_sub_or_wave<FAM, HSRLE_S, AL>(a, SB, 0u, rec, st); }

#define HSRLE_DEF_MAIN(FAM, AL, TAG)                                                                                                   \
  static hipError_t dec_##TAG(const DecodeArgs &a, hipStream_t st) { return HSRLE_DECODE_LAUNCH(FAM, AL); } \
  static hipError_t enc_##TAG(const EncodeArgs &a, hipStream_t st) { return HSRLE_ENCODE_LAUNCH_RL(FAM, AL); } \
  static hipError_t idx_##TAG(const IndexArgs &a, int records, hipStream_t st) { return launch_index<FAM, HSRLE_S, AL>(a, records, st); } \
  static hipError_t sub_##TAG(const DecodeArgs &a, uint32_t SB, uint32_t *rec, hipStream_t st) { return launch_sub_or_wave<FAM, HSRLE_S, AL>(a, SB, 0u, rec, st); }

HSRLE_DEF_MAIN(PLAIN, 1, sym)
HSRLE_DEF_MAIN(PACKED, 1, sym_packed)
HSRLE_DEF_MAIN(LUT3, 1, lut3_sym)
HSRLE_DEF_MAIN(LUT7, 1, lut7_sym)
HSRLE_DEF_MAIN(PLAIN, 0, byte)
HSRLE_DEF_MAIN(PACKED, 0, byte_packed)
HSRLE_DEF_MAIN(LUT3, 0, lut3_byte)
HSRLE_DEF_MAIN(LUT7, 0, lut7_byte)
// Short family (reference: src/rle.h:226-348)
HSRLE_DEF_MAIN(SHORT0, 1, short0_sym)
HSRLE_DEF_MAIN(SHORT1, 1, short1_sym)
HSRLE_DEF_MAIN(SHORT3, 1, short3_sym)
HSRLE_DEF_MAIN(SHORT7, 1, short7_sym)
HSRLE_DEF_MAIN(SHORT0, 0, short0_byte)
HSRLE_DEF_MAIN(SHORT1, 0, short1_byte)
HSRLE_DEF_MAIN(SHORT3, 0, short3_byte)
HSRLE_DEF_MAIN(SHORT7, 0, short7_byte)

// chunks of ONE monolithic stream (hsrle_mono_encode.hip.h): the list-free codecs of this width
#define HSRLE_DEF_MONO(FAM, AL, TAG) \
  static hipError_t menc_##TAG(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st) { return launch_mono_encode(k_encodeS_blocks<FAM, HSRLE_S, AL, true>, a, m, st); }
HSRLE_DEF_MONO(PLAIN, 1, sym)
HSRLE_DEF_MONO(PACKED, 1, sym_packed)
HSRLE_DEF_MONO(PLAIN, 0, byte)
HSRLE_DEF_MONO(PACKED, 0, byte_packed)
HSRLE_DEF_MONO(SHORT0, 1, short0_sym)
HSRLE_DEF_MONO(SHORT0, 0, short0_byte)
// ... and the codecs with a move-to-front list (the list in front of a chunk is guessed, checked and repaired: hsrle_capi.hip)
HSRLE_DEF_MONO(LUT3, 1, lut3_sym)
HSRLE_DEF_MONO(LUT7, 1, lut7_sym)
HSRLE_DEF_MONO(LUT3, 0, lut3_byte)
HSRLE_DEF_MONO(LUT7, 0, lut7_byte)
HSRLE_DEF_MONO(SHORT1, 1, short1_sym)
HSRLE_DEF_MONO(SHORT3, 1, short3_sym)
HSRLE_DEF_MONO(SHORT7, 1, short7_sym)
HSRLE_DEF_MONO(SHORT1, 0, short1_byte)
HSRLE_DEF_MONO(SHORT3, 0, short3_byte)
HSRLE_DEF_MONO(SHORT7, 0, short7_byte)

// Greedy encoders of the byte-aligned LUT Short codecs (reference: src/rle.h:398-416); decode = the Short decoder of the grammar.
// No residency cap: the per-lane output path (byte stores, global literal copies) still waits on memory, more resident waves help.
static hipError_t enc_greedy1(const EncodeArgs &a, hipStream_t st) { return launch_encode(k_encode_greedy_blocks<SHORT1, HSRLE_S>, a, st, 0); }
static hipError_t enc_greedy3(const EncodeArgs &a, hipStream_t st) { return launch_encode(k_encode_greedy_blocks<SHORT3, HSRLE_S>, a, st, 0); }
static hipError_t enc_greedy7(const EncodeArgs &a, hipStream_t st) { return launch_encode(k_encode_greedy_blocks<SHORT7, HSRLE_S>, a, st, 0); }
// ... and their chunks of ONE monolithic stream (round 4: the drop-in *_compress_greedy by many lanes)
static hipError_t menc_greedy1(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st) { return launch_mono_encode(k_encode_greedy_blocks<SHORT1, HSRLE_S, true>, a, m, st); }
static hipError_t menc_greedy3(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st) { return launch_mono_encode(k_encode_greedy_blocks<SHORT3, HSRLE_S, true>, a, m, st); }
static hipError_t menc_greedy7(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st) { return launch_mono_encode(k_encode_greedy_blocks<SHORT7, HSRLE_S, true>, a, m, st); }

void HSRLE_CAT(register_w, HSRLE_W)(DecodeLaunch *dec, EncodeLaunch *enc, IndexLaunch *idx, SubBlockLaunch *sub, MonoEncodeLaunch *menc)
{
  // one line per codec: the slot of <FAM, HSRLE_S, AL> (hsrle_codecs.h) in every table
#define HSRLE_REG(FAM, AL, TAG) \
  { constexpr int c = codec_id(FAM, HSRLE_S, AL); dec[c] = dec_##TAG; idx[c] = idx_##TAG; sub[c] = sub_##TAG; enc[c] = enc_##TAG; menc[c] = menc_##TAG; }
  HSRLE_REG(PLAIN, 1, sym) HSRLE_REG(PACKED, 1, sym_packed) HSRLE_REG(LUT3, 1, lut3_sym) HSRLE_REG(LUT7, 1, lut7_sym)
  HSRLE_REG(PLAIN, 0, byte) HSRLE_REG(PACKED, 0, byte_packed) HSRLE_REG(LUT3, 0, lut3_byte) HSRLE_REG(LUT7, 0, lut7_byte)
  HSRLE_REG(SHORT0, 1, short0_sym) HSRLE_REG(SHORT1, 1, short1_sym) HSRLE_REG(SHORT3, 1, short3_sym) HSRLE_REG(SHORT7, 1, short7_sym)
  HSRLE_REG(SHORT0, 0, short0_byte) HSRLE_REG(SHORT1, 0, short1_byte) HSRLE_REG(SHORT3, 0, short3_byte) HSRLE_REG(SHORT7, 0, short7_byte)
#undef HSRLE_REG
  // Greedy: encoders of their own, the Short decoders of the same grammar
#define HSRLE_REG_GREEDY(FAM, K) \
  { constexpr int c = codec_id(FAM, HSRLE_S, 0, true); dec[c] = dec_short##K##_byte; idx[c] = idx_short##K##_byte; sub[c] = sub_short##K##_byte; enc[c] = enc_greedy##K; menc[c] = menc_greedy##K; }
  HSRLE_REG_GREEDY(SHORT1, 1) HSRLE_REG_GREEDY(SHORT3, 3) HSRLE_REG_GREEDY(SHORT7, 7)
#undef HSRLE_REG_GREEDY
}

} // namespace hsrle
