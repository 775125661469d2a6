// hsrle_inst_generic.inc -- instantiates the codecs of one symbol width (16/24/32/48/64 bit): 8 extreme, 8 Short, 3 Greedy.
// Included by inst_wNN.hip with HSRLE_S (symbol bytes) defined.
#include "hsrle_decode.hip.h"
#include "hsrle_encode.hip.h"
#include "hsrle_encodeS.hip.h"
#include "hsrle_encode_greedy.hip.h"
#include "hsrle_index.hip.h"
#include "hsrle_launch.h"

namespace hsrle {

constexpr int kS = HSRLE_S;

// Decode: launch_decode_codec (hsrle_launch.h) by the rule of hsrle_codecs.h (decode_variant) -- the row says whether the width has a 64-byte stream ring.

// Round 6: every codec of 2 .. 8 byte symbols except Greedy is position-parallel for blocks up to 4 KiB (hsrle_codecs.h: encode_choice) -- the run list encoders of
// these widths (small containers of 1 .. 4 KiB blocks, and big containers of 3 / 4 byte symbols on run-distributed data) had nothing left to take and are gone.
// What is launched here: blocks above 4 KiB.
// 2 byte symbols: the history ring is chosen per input (launch_encode_ring, hsrle_launch.h); wider ones always use 128 bytes.  A/B builds: HSRLE_ENCODE_V1 selects the
// first-generation encoder (hsrle_encode.hip.h), HSRLE_ENCS_RING one ring for every width and input.
template <int FAM, int AL>
static hipError_t enc_launch(const EncodeArgs &a, hipStream_t st)
{
  if constexpr (kEncodeV1) return launch_encode(k_encode_blocks<FAM, kS, AL>, a, st, 0);
  else if constexpr (kS == 2 && !kEncSRingFixed) return launch_encode_ring<2>(k_encodeS_blocks<FAM, 2, AL, false, 256>, k_encodeS_blocks<FAM, 2, AL, false, 128>, a, st);
  else return launch_encode(k_encodeS_blocks<FAM, kS, AL>, a, st, 0);
}
// chunks of ONE monolithic stream (hsrle_mono_encode.hip.h): the list-free codecs, and the codecs with a move-to-front list (the list in front of a chunk is
// guessed, checked and repaired: hsrle_capi_mono_encode.h)
template <int FAM, int AL>
static hipError_t menc_launch(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st) { return launch_mono_encode(k_encodeS_blocks<FAM, kS, AL, true>, a, m, st); }
template <int FAM, int AL>
static hipError_t sub_launch(const DecodeArgs &a, uint32_t SB, uint32_t *rec, hipStream_t st) { return launch_sub_or_wave<FAM, kS, AL>(a, SB, 0u, rec, st); }

// Greedy encoders of the byte-aligned LUT Short codecs (reference: src/rle.h:398-416); decode = the Short decoder of the grammar.
// No residency cap: the per-lane output path (byte stores, global literal copies) still waits on memory, more resident waves help.
template <int FAM>
static hipError_t enc_greedy(const EncodeArgs &a, hipStream_t st) { return launch_encode(k_encode_greedy_blocks<FAM, kS>, a, st, 0); }
// ... and their chunks of ONE monolithic stream (round 4: the drop-in *_compress_greedy by many lanes)
template <int FAM>
static hipError_t menc_greedy(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st) { return launch_mono_encode(k_encode_greedy_blocks<FAM, kS, true>, a, m, st); }

// the row of <FAM, HSRLE_S, AL> (hsrle_codecs.h); a Greedy row: encoders of its own, decoder and index passes of the Short grammar
template <int FAM, int AL, bool GREEDY = false>
static void reg(CodecLaunch *t)
{
  constexpr int c = codec_id(FAM, kS, AL, GREEDY);
  t[c].dec = launch_decode_codec<c>;
  t[c].idx = launch_index<FAM, kS, AL>;
  t[c].sub = sub_launch<FAM, AL>;
  if constexpr (GREEDY) { t[c].enc = enc_greedy<FAM>; t[c].menc = menc_greedy<FAM>; }
  else { t[c].enc = enc_launch<FAM, AL>; t[c].menc = menc_launch<FAM, AL>; }
}
template <int AL>
static void reg_aligned(CodecLaunch *t)
{
  reg<PLAIN, AL>(t); reg<PACKED, AL>(t); reg<LUT3, AL>(t); reg<LUT7, AL>(t);
  reg<SHORT0, AL>(t); reg<SHORT1, AL>(t); reg<SHORT3, AL>(t); reg<SHORT7, AL>(t);      // Short family (reference: src/rle.h:226-348)
}

static void register_width(CodecLaunch *t)   // (the unit gives it its name: register_wNN)
{
  reg_aligned<1>(t); reg_aligned<0>(t);
  reg<SHORT1, 0, true>(t); reg<SHORT3, 0, true>(t); reg<SHORT7, 0, true>(t);
}

} // namespace hsrle
