// 128 bit symbols: rle128_{sym,byte}[_packed]  (reference: src/rle.h:124-125, :146-147, :168-169, :194-195)
#include "hsrle_decode.hip.h"
#include "hsrle_encode.hip.h"
#include "hsrle_encode128.hip.h"
#include "hsrle_index.hip.h"
#include "hsrle_launch.h"

namespace hsrle {

// ring encoder (hsrle_encode128.hip.h) for block sizes up to 64 KiB; HSRLE_ENCODE128_V1=1 selects the first-generation kernel (A/B runs)
template <int FAM, int AL>
static hipError_t enc_any(const EncodeArgs &a, hipStream_t st)
{
  static const bool v1 = knob_u32("HSRLE_ENCODE128_V1", 0u) != 0u;
  if (v1 || a.B > 65536u) return launch_encode(k_encode_blocks<FAM, 16, AL>, a, st);   // (the one-block drop-in path spans the whole input with one block: one lane either way)
  return launch_encode(k_encode128_blocks<FAM == PACKED, AL>, a, st, 0);
}
template <int FAM, int AL>
static hipError_t sub_launch(const DecodeArgs &a, uint32_t SB, uint32_t *rec, hipStream_t st) { return launch_sub_or_wave<FAM, 16, AL>(a, SB, 0u, rec, st); }

// chunks of one monolithic stream (hsrle_mono_encode.hip.h): the first-generation encoder, one lane per chunk, from its place behind a stored run
template <int FAM, int AL>
static hipError_t menc_any(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st)
{
  hipLaunchKernelGGL((k_encode128_chunks<FAM, AL>), dim3((a.nBlocks + 63u) / 64u), dim3(64), 0, st, a.in, a.U, a.nBlocks, m.starts, m.syms, m.slotOff, a.slots, a.sizes, a.B, (const uint32_t *)a.ringSel);
  return hipGetLastError();
}

// the row of <FAM, 16, AL> (hsrle_codecs.h); its decoder by the rule of hsrle_codecs.h (decode_variant): no 64-byte ring at this width
template <int FAM, int AL>
static void reg(CodecLaunch *t)
{
  constexpr int c = codec_id(FAM, 16, AL);
  t[c].dec = launch_decode_codec<c>;
  t[c].enc = enc_any<FAM, AL>;
  t[c].idx = launch_index<FAM, 16, AL>;
  t[c].sub = sub_launch<FAM, AL>;
  t[c].menc = menc_any<FAM, AL>;
}

void register_w128(CodecLaunch *t) { reg<PLAIN, 1>(t); reg<PACKED, 1>(t); reg<PLAIN, 0>(t); reg<PACKED, 0>(t); }

} // namespace hsrle
