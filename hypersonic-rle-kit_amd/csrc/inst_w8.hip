// 8 bit symbols: rle8_multi / rle8_single / rle8_packed_multi / rle8_packed_single / rle8_{3,7}symlut
// (reference: src/rle.h:101-103, :173-175, :199-208).  rle8_decompress / rle8_packed_decompress decode both the multi
// and the single mode, so the Single codec ids share the multi decode kernels.
#include "hsrle_decode.hip.h"
#ifdef HSRLE_DEC8_PE
#include "experiments/hsrle_decode8pe.hip.h"
#endif
#include "hsrle_encode.hip.h"
#include "hsrle_encode8.hip.h"
#include "hsrle_encode8r.hip.h"
#ifdef HSRLE_EXPERIMENTS
#include "experiments/hsrle_encode8w.hip.h"        // one wave per block: bit-exact, measured slower
#endif
#include "hsrle_encode8s.hip.h"
#include "hsrle_encode_greedy.hip.h"
#include "hsrle_index.hip.h"
#include "hsrle_launch.h"

namespace hsrle {

// Decode: ids 0 / 1 (rle8_multi, rle8_packed_multi) take the kernel without the Single mode, their encoders only write mode 0; ids 4 / 5 (the Single codecs) and any
// stream whose mode byte says 1 (hsrle_capi.hip: mono_decompress) the general kernel -- hsrle_codecs.h: decode_variant, launched by launch_decode_codec (hsrle_launch.h)

// rle8_multi / rle8_packed_multi / rle8_3symlut / rle8_7symlut: the ring encoder (one lane per block) for containers that fill the device with it, the run list encoder
// (hsrle_encode8r.hip.h: the whole wave per block) for smaller ones of 1 .. 4 KiB blocks.  Experiment builds: HSRLE_RUNLIST=1 / 2 = always / never.
template <int FAM>
static hipError_t enc_multi8(const EncodeArgs &a, hipStream_t st)
{
  // (round 6: plain / Packed / Short without and with a one-symbol list are position-parallel for every block the run list encoder took)
  if constexpr (FAM == SHORT3 || FAM == SHORT7)
  {
    static const uint32_t force = knob_u32("HSRLE_RUNLIST", 0u);
    if (run_list_applies(a.nBlocks, a.B, a.U, force) && a.residentWorkgroups == nullptr)
      return launch_run_list(k_encode8_runlist<FAM>, a, st);
  }
  return launch_encode_ring<1>(k_encode8_blocks<FAM, false, 256>, k_encode8_blocks<FAM, false, 128>, a, st);
}
// the blocks' symbols by one wave per block (k_single_pick holds a block in dynamic LDS: table, the block padded to 64, the equality bits)
static hipError_t single_pick_launch(const EncodeArgs &a, uint8_t *syms, uint32_t symStride, uint32_t symAt, const MonoEncodeArgs &m, hipStream_t st)
{
  const uint32_t padded = (a.B + 63u) & ~63u;
  const uint32_t lds = 1024u + padded + 64u + (padded / 64u + 1u) * 8u;
  hipLaunchKernelGGL(k_single_pick, dim3(a.nBlocks), dim3(64), lds, st, a.in, a.U, a.B, a.nBlocks, syms, symStride, symAt, m.cutPos, m.cutSym, m.cutFlags, m.cutG, m.cutLong);
  return hipGetLastError();
}
// split encode of a container, phase 1: the blocks' symbols (a byte per block; a.nBlocks = blocks here) and their cuts -- the cut finder needs the symbols
static hipError_t single_pick_phase(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st)
{
  if (a.B > kSinglePickMaxBlock) return hipErrorInvalidValue;
  return single_pick_launch(a, (uint8_t *)const_cast<uint32_t *>(m.pick), 1u, 0u, m, st);
}
// Single: symbol pick by one wave per block, then the ring encoder (hsrle_encode8s.hip.h).  Blocks above kSinglePickMaxBlock (the one-lane
// drop-in path spans the whole input with one block) and HSRLE_SINGLE_V1=1 (A/B runs) use the first-generation kernel.
template <int MODE>   // 0 rle8_single, 1 rle8_packed_single, 2 rle8_single_short
static hipError_t enc_single_any(const EncodeArgs &a, hipStream_t st)
{
  static const bool v1 = knob_u32("HSRLE_SINGLE_V1", 0u) != 0u;
  if (v1 || a.B > kSinglePickMaxBlock)
  {
    if constexpr (MODE == 2) return launch_encode(k_encode_single_short_blocks<SHORT_SINGLE>, a, st, 0);
    else return launch_encode(k_encode_blocks<MODE == 1 ? PACKED_SINGLE : SINGLE, 1, 0>, a, st, 0);   // no residency cap: +40 % on run data, +20 % on noise, -8 % on video-shaped
  }
  if (a.residentWorkgroups == nullptr && single_pick_launch(a, a.slots, a.slotStride, MODE == 2 ? 8u : 9u, MonoEncodeArgs{}, st) != hipSuccess)
    return hipErrorLaunchFailure;
  return launch_encode(k_encode8_single_blocks<MODE>, a, st, 0);
}

template <int FAM>
static hipError_t menc_multi8(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st) { return launch_mono_encode(k_encode8_blocks<FAM, true>, a, m, st); }
// rle8_single_short as chunks of one monolithic stream (round 4; hsrle_encode_greedy.hip.h)
static hipError_t menc_single_short(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st)
{
  if (m.phase == 1u) return single_pick_phase(a, m, st);
  hipLaunchKernelGGL((k_encode_single_short_chunks<SHORT_SINGLE>), dim3((a.nBlocks + 63u) / 64u), dim3(64), 0, st, a.in, a.U, a.nBlocks, m.starts, m.slotOff, a.slots, a.sizes, m.pick,
                     m.jobs, m.jobCount, m.jobCap, a.B, (const uint32_t *)a.ringSel);
  if (m.jobs != nullptr)
    hipLaunchKernelGGL((k_copy_jobs<0>), dim3(2048), dim3(256), 0, st, a.in, a.slots, (const uint64_t *)m.jobs, (const uint32_t *)m.jobCount, m.jobCap);
  return hipGetLastError();
}
// 8 bit Single as chunks of one monolithic stream: the first-generation scanner, one lane per chunk (hsrle_encode.hip.h)
template <bool PACKEDSINGLE>
static hipError_t menc_single_any(const EncodeArgs &a, const MonoEncodeArgs &m, hipStream_t st)
{
  if (m.phase == 1u) return single_pick_phase(a, m, st);
  hipLaunchKernelGGL((k_encode_single_chunks<PACKEDSINGLE>), dim3((a.nBlocks + 63u) / 64u), dim3(64), 0, st, a.in, a.U, a.nBlocks, m.starts, m.slotOff, a.slots, a.sizes, m.pick,
                     m.jobs, m.jobCount, m.jobCap, a.B, (const uint32_t *)a.ringSel);
  if (m.jobs != nullptr)
    hipLaunchKernelGGL((k_copy_jobs<0>), dim3(2048), dim3(256), 0, st, a.in, a.slots, (const uint64_t *)m.jobs, (const uint32_t *)m.jobCount, m.jobCap);
  return hipGetLastError();
}
#ifdef HSRLE_EXPERIMENTS
static hipError_t wenc_plain(const WaveEncodeArgs &a, hipStream_t st) { return launch_wave_encode(k_encode8_wave<PLAIN>, a, st); }
static hipError_t wenc_packed(const WaveEncodeArgs &a, hipStream_t st) { return launch_wave_encode(k_encode8_wave<PACKED>, a, st); }
#endif

template <int FAM, uint32_t ALLOW_SINGLE>
static hipError_t sub_launch(const DecodeArgs &a, uint32_t SB, uint32_t *rec, hipStream_t st) { return launch_sub_or_wave<FAM, 1, 0>(a, SB, ALLOW_SINGLE, rec, st); }

// the row of <FAM, 1, 0> (hsrle_codecs.h): the decoder its row names, index and sub-block passes of the kernel family KFAM (the Single ids: the multi kernels' general form)
template <int FAM, int KFAM = FAM>
static void reg(CodecLaunch *t, EncodeLaunch enc, MonoEncodeLaunch menc)
{
  constexpr int c = codec_id(FAM, 1, 0);
  static_assert(decode_variant(kCodecs[c], false, false, false).fam == KFAM, "index and sub-block passes of another grammar than the decoder's");
  t[c].dec = launch_decode_codec<c>;
  t[c].idx = launch_index<KFAM, 1, 0>;
  t[c].sub = sub_launch<KFAM, FAM != KFAM ? 1u : 0u>;
  t[c].enc = enc;
  t[c].menc = menc;
}
template <int FAM>
static void reg_multi(CodecLaunch *t) { reg<FAM>(t, enc_multi8<FAM>, menc_multi8<FAM>); }

void register_w8(CodecLaunch *t)
{
#ifdef HSRLE_EXPERIMENTS
  t[codec_id(PLAIN, 1, 0)].wenc = wenc_plain; t[codec_id(PACKED, 1, 0)].wenc = wenc_packed;
#endif
  reg_multi<PLAIN>(t); reg_multi<PACKED>(t); reg_multi<LUT3>(t); reg_multi<LUT7>(t);
  reg<SINGLE, PLAIN>(t, enc_single_any<0>, menc_single_any<false>);
  reg<PACKED_SINGLE, PACKED>(t, enc_single_any<1>, menc_single_any<true>);
  // Short family (rle8_multi_short, rle8_{1,3,7}symlut_short; reference: src/rle.h:202-222) and rle8_single_short (src/rle.h:223-224)
  reg_multi<SHORT0>(t); reg_multi<SHORT1>(t); reg_multi<SHORT3>(t); reg_multi<SHORT7>(t);
  reg<SHORT_SINGLE>(t, enc_single_any<2>, menc_single_short);
}

} // namespace hsrle

#ifdef HSRLE_ENC_STAMPS
extern "C" int hsrle_debug_enc_stamps(unsigned long long *out, int reset)
{
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(hsrle::g_enc_stamps), sizeof(hsrle::g_enc_stamps)) != hipSuccess) return 1;
  if (reset) { unsigned long long z[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }; if (hipMemcpyToSymbol(HIP_SYMBOL(hsrle::g_enc_stamps), z, sizeof(z)) != hipSuccess) return 1; }
  return 0;
}
#endif
