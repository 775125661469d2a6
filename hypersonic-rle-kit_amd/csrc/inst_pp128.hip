// inst_pp128.hip -- instantiations of the position-parallel 128 bit encoder (hsrle_encode128p.hip.h): rle128_sym, rle128_sym_packed, rle128_byte, rle128_byte_packed
#include "hsrle_launch.h"
#include "hsrle_encode128p.hip.h"

namespace hsrle {

template <bool PK, int AL>
static hipError_t pp128_launch(const PpArgs &a, int phase, hipStream_t st)
{
  const PpScratch sc = pp_scratch_of(a);
  if (phase == 0)
    hipLaunchKernelGGL((k_encode128_pp<PK, AL, 0>), dim3(a.nBlocks), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.sizes, a.offsets, a.payload, sc);
  else
    hipLaunchKernelGGL((k_encode128_pp<PK, AL, 1>), dim3(a.nBlocks), dim3(64), 0, st, a.in, a.U, a.B, a.nBlocks, a.sizes, a.offsets, a.payload, sc);
  return hipGetLastError();
}

void register_pp128(CodecLaunch *t)
{
  t[codec_id(PLAIN, 16, 1)].pp = pp128_launch<false, 1>;
  t[codec_id(PACKED, 16, 1)].pp = pp128_launch<true, 1>;
  t[codec_id(PLAIN, 16, 0)].pp = pp128_launch<false, 0>;
  t[codec_id(PACKED, 16, 0)].pp = pp128_launch<true, 0>;
}

} // namespace hsrle
