// inst_pp8.hip -- instantiations of the position-parallel 8 bit encoder (hsrle_encode8p.hip.h): rle8_multi, rle8_packed_multi
#include "hsrle_launch.h"
#include "hsrle_encode8p.hip.h"

namespace hsrle {

template <int FAM>
static hipError_t pp_launch(const PpArgs &a, int phase, hipStream_t st)
{
  PpScratch sc = pp_scratch_of(a);
  sc.stamps = a.scratch + ((pp_scratch_bytes(a.nBlocks, a.B) + 255ull) & ~255ull);   // (diagnostic builds: 128 bytes per block behind the scratch, in the caller's slot area)
  if (phase == 0)
    hipLaunchKernelGGL((k_encode8_pp<FAM, 0>), dim3((a.nBlocks + kPp8Bpw - 1u) / kPp8Bpw), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.sizes, a.offsets, a.payload, sc);
  else
    hipLaunchKernelGGL((k_encode8_pp<FAM, 1>), dim3((a.nBlocks + kPp8Bpw - 1u) / kPp8Bpw), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.sizes, a.offsets, a.payload, sc);
  return hipGetLastError();
}

void register_pp8(CodecLaunch *t)
{
  t[codec_id(PLAIN, 1, 0)].pp = pp_launch<PLAIN>;
  t[codec_id(PACKED, 1, 0)].pp = pp_launch<PACKED>;
}

} // namespace hsrle
