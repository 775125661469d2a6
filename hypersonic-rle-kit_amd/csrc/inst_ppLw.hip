// inst_ppLw.hip -- instantiations of the windowed position-parallel LUT encoder (hsrle_encodeLpw.hip.h): the codecs of inst_ppL.hip, blocks above 4 KiB
#include "hsrle_launch.h"
#include "hsrle_encodeLpw.hip.h"

namespace hsrle {

template <int FAM, int S, int AL>
static hipError_t ppL_launch(const PpwArgs &a, int phase, hipStream_t st)
{
  if (phase == 0)
    hipLaunchKernelGGL((k_encodeL_ppw_scan<FAM, S, AL>), dim3(a.nUnits), dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL((k_encodeL_ppw_emit<FAM, S, AL>), dim3(a.nWindows), dim3(64), 0, st, a);
  return hipGetLastError();
}

// the slot of <FAM, S, AL> in a table by codec id (hsrle_codecs.h)
template <int FAM, int S, int AL>
static void reg(CodecLaunch *t) { t[codec_id(FAM, S, AL)].ppwL = ppL_launch<FAM, S, AL>; }

// the 7 symbol LUT codecs of one width, sym- and byte-aligned
template <int S>
static void reg_lut7(CodecLaunch *t) { reg<LUT7, S, 1>(t); reg<LUT7, S, 0>(t); }

// Short family with a list of 3 / 7 symbols (the three-symbol list of 6 / 8 byte symbols has its closed form in hsrle_encodeSp.hip.h)
template <int S>
static void reg_short37(CodecLaunch *t)
{
  if constexpr (S <= 4) { reg<SHORT3, S, 1>(t); reg<SHORT3, S, 0>(t); }
  reg<SHORT7, S, 1>(t); reg<SHORT7, S, 0>(t);
}

void register_ppLw(CodecLaunch *t)
{
  // (rle8_3symlut_short / rle8_7symlut_short stay with the ring / run list encoders: with 8 bit symbols every PAIR of equal bytes is a candidate -- a second round for
  //  a handful of them on run data, 280 candidates per block on video-shaped data -- measured 1 355 / 632 and 956 / 705 GiB/s against 1 134 / 1 221 and 1 126 / 1 173)
  reg_short37<2>(t); reg_short37<3>(t); reg_short37<4>(t); reg_short37<6>(t); reg_short37<8>(t);
  reg<LUT3, 1, 0>(t); reg<LUT7, 1, 0>(t);      // rle8_3symlut, rle8_7symlut
  reg<LUT3, 2, 1>(t); reg<LUT3, 2, 0>(t);      // rle16_3symlut_sym, rle16_3symlut_byte
  reg_lut7<2>(t); reg_lut7<3>(t); reg_lut7<4>(t); reg_lut7<6>(t); reg_lut7<8>(t);
}

} // namespace hsrle
