// inst_ppSw.hip -- instantiations of the windowed position-parallel encoder of 1 .. 8 byte symbols (hsrle_encodeSpw.hip.h): the codecs of inst_ppS.hip, blocks above 4 KiB;
// and its chunk mode (MONO) for the chunks of one monolithic stream: the plain / Packed codecs and the Short codecs with no list or a one-symbol list
#include "hsrle_launch.h"
#include "hsrle_encodeSpw.hip.h"

namespace hsrle {

template <int FAM, int S, int AL, bool MONO = false>
static hipError_t ppS_launch(const PpwArgs &a, int phase, hipStream_t st)
{
  if (phase == 0)
    hipLaunchKernelGGL((k_encodeS_ppw_scan<FAM, S, AL, MONO>), dim3(a.nUnits), dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL((k_encodeS_ppw_emit<FAM, S, AL, MONO>), dim3(a.nWindows), dim3(64), 0, st, a);
  return hipGetLastError();
}

// the slot of <FAM, S, AL> in a table by codec id (hsrle_codecs.h)
template <int FAM, int S, int AL, bool MONO = false>
static void reg(CodecLaunch *t)
{
  if constexpr (MONO) t[codec_id(FAM, S, AL)].ppwSM = ppS_launch<FAM, S, AL, true>;
  else t[codec_id(FAM, S, AL)].ppwS = ppS_launch<FAM, S, AL, false>;
}

// plain and Packed, sym- and byte-aligned, of one width
template <int S>
static void reg_width(CodecLaunch *t) { reg<PLAIN, S, 1>(t); reg<PACKED, S, 1>(t); reg<PLAIN, S, 0>(t); reg<PACKED, S, 0>(t); }

// ... the 3 symbol LUT codecs: symbols of 3 bytes and more (hsrle_encodeSp.hip.h)
template <int S>
static void reg_lut3(CodecLaunch *t) { reg<LUT3, S, 1>(t); reg<LUT3, S, 0>(t); }

// Short family without a list / with a one-symbol list: the chain of the emit decisions runs through (lastRLE, last stored symbol) as it does for plain / Packed
template <int S>
static void reg_short(CodecLaunch *t) { reg<SHORT0, S, 1>(t); reg<SHORT1, S, 1>(t); reg<SHORT0, S, 0>(t); reg<SHORT1, S, 0>(t); }

// ... with a three-symbol list: 6 and 8 byte symbols (every run stored: hsrle_encodeSp.hip.h)
template <int S>
static void reg_short3(CodecLaunch *t) { reg<SHORT3, S, 1>(t); reg<SHORT3, S, 0>(t); }

// chunk mode: the codecs whose encoder state at a cut is fixed by the cut (no list, or a list of one symbol; hsrle_codecs.h: chunk_mode)
template <int S>
static void reg_mono(CodecLaunch *t)
{
  reg<PLAIN, S, 1, true>(t); reg<PACKED, S, 1, true>(t); reg<PLAIN, S, 0, true>(t); reg<PACKED, S, 0, true>(t);
  reg<SHORT0, S, 1, true>(t); reg<SHORT1, S, 1, true>(t); reg<SHORT0, S, 0, true>(t); reg<SHORT1, S, 0, true>(t);
}

void register_ppSw(CodecLaunch *t)
{
  reg<SHORT0, 1, 0, true>(t); reg<SHORT1, 1, 0, true>(t);      // chunk mode: rle8_multi_short, rle8_1symlut_short
  reg_mono<2>(t); reg_mono<3>(t); reg_mono<4>(t); reg_mono<6>(t); reg_mono<8>(t);
  reg_short3<6>(t); reg_short3<8>(t);
  reg<SHORT0, 1, 0>(t); reg<SHORT1, 1, 0>(t);      // rle8_multi_short, rle8_1symlut_short
  reg_short<2>(t); reg_short<3>(t); reg_short<4>(t); reg_short<6>(t); reg_short<8>(t);
  reg_width<2>(t); reg_width<3>(t); reg_width<4>(t); reg_width<6>(t); reg_width<8>(t);
  reg_lut3<3>(t); reg_lut3<4>(t); reg_lut3<6>(t); reg_lut3<8>(t);
}

} // namespace hsrle
