// inst_ppS.hip -- instantiations of the position-parallel encoder of 2 .. 8 byte symbols (hsrle_encodeSp.hip.h): plain and Packed, sym- and byte-aligned
#include "hsrle_launch.h"
#include "hsrle_encodeSp.hip.h"

namespace hsrle {

template <int FAM, int S, int AL>
static hipError_t ppS_launch(const PpArgs &a, int phase, hipStream_t st)
{
  const PpScratch sc = pp_scratch_of(a);
  if (phase == 0)
    hipLaunchKernelGGL((k_encodeS_pp<FAM, S, AL, 0>), dim3(a.nBlocks), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.sizes, a.offsets, a.payload, sc);
  else
    hipLaunchKernelGGL((k_encodeS_pp<FAM, S, AL, 1>), dim3(a.nBlocks), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.sizes, a.offsets, a.payload, sc);
  return hipGetLastError();
}

// the slot of <FAM, S, AL> in a table by codec id (hsrle_codecs.h)
template <int FAM, int S, int AL>
static void reg(CodecLaunch *t) { t[codec_id(FAM, S, AL)].pp = ppS_launch<FAM, S, AL>; }

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

void register_ppS(CodecLaunch *t)
{
  reg_short3<6>(t); reg_short3<8>(t);
  reg<SHORT0, 1, 0>(t); reg<SHORT1, 1, 0>(t);      // rle8_multi_short, rle8_1symlut_short
  reg_short<2>(t); reg_short<3>(t); reg_short<4>(t); reg_short<6>(t); reg_short<8>(t);
  reg_width<2>(t); reg_width<3>(t); reg_width<4>(t); reg_width<6>(t); reg_width<8>(t);
  reg_lut3<3>(t); reg_lut3<4>(t); reg_lut3<6>(t); reg_lut3<8>(t);
}

} // namespace hsrle
