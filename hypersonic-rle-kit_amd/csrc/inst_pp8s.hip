// inst_pp8s.hip -- instantiations of the position-parallel 8 bit Single encoder (hsrle_encode8sp.hip.h): rle8_single, rle8_packed_single, rle8_single_short
#include "hsrle_launch.h"
#include "hsrle_encode8sp.hip.h"

namespace hsrle {

template <int CODEC>
static hipError_t pps_launch(const PpArgs &a, int phase, hipStream_t st)
{
  const PpScratch sc = pp_scratch_of(a);
  if (phase == 0)
    hipLaunchKernelGGL((k_encode8s_pp<CODEC, 0>), dim3(a.nBlocks), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.sizes, a.offsets, a.payload, sc);
  else
    hipLaunchKernelGGL((k_encode8s_pp<CODEC, 1>), dim3(a.nBlocks), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.sizes, a.offsets, a.payload, sc);
  return hipGetLastError();
}

void register_pp8s(CodecLaunch *t)
{
  t[codec_id(SINGLE, 1, 0)].pp = pps_launch<0>;
  t[codec_id(PACKED_SINGLE, 1, 0)].pp = pps_launch<1>;
  t[codec_id(SHORT_SINGLE, 1, 0)].pp = pps_launch<2>;
}

} // namespace hsrle
