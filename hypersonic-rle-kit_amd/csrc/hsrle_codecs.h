// hsrle_codecs.h -- what every codec IS, said once: one row per codec id (include/hsrle.h: hsrle_codec_t), and the facts the host code derives from a row.
// Host-only and free of HIP: a plain C++17 compiler can include it (tests/test_codec_traits.py does).  The kernels are instantiated as <FAM, S, AL>
// (hsrle_common.hip.h: Traits); codec_id() is the way from those template arguments to the slot of a launch table.
#pragma once
#include "../../include/hsrle.h"

#include <stdint.h>

namespace hsrle {

enum Family : int { PLAIN = 0, PACKED = 1, LUT3 = 2, LUT7 = 3, SINGLE = 4, PACKED_SINGLE = 5,
                    SHORT0 = 6, SHORT1 = 7, SHORT3 = 8, SHORT7 = 9,     // Short family: 0 / 1 / 3 / 7 symbol LUT, one-byte packed headers
                    SHORT_SINGLE = 10 };                                // rle8_single_short: one symbol per stream, none in the packets

struct CodecInfo
{
  const char *name;   // names follow the reference: src/rle.h, src/codec_funcs.h:270-410
  Family fam;
  uint8_t S;          // symbol bytes
  uint8_t aligned;    // sym-aligned (1) or byte-aligned (0); 0 for 8 bit symbols
  bool greedy;        // a Greedy ENCODER of the family's grammar
};

constexpr int kCodecCount = 110;                 // 50 extreme codecs + 44 of the Short family + 15 Greedy encoders (8f-1) + rle8_single_short
constexpr CodecInfo kCodecs[kCodecCount] = {
  // 8 bit symbols (reference: src/rle.h:101-103, :173-175, :199-208)
  { "rle8_multi", PLAIN, 1, 0, false }, { "rle8_packed_multi", PACKED, 1, 0, false }, { "rle8_3symlut", LUT3, 1, 0, false },
  { "rle8_7symlut", LUT7, 1, 0, false }, { "rle8_single", SINGLE, 1, 0, false }, { "rle8_packed_single", PACKED_SINGLE, 1, 0, false },
  // 2 .. 8 byte symbols, per width: sym-aligned plain / Packed / 3 / 7 symbol LUT, then the byte-aligned four
  { "rle16_sym", PLAIN, 2, 1, false }, { "rle16_sym_packed", PACKED, 2, 1, false }, { "rle16_3symlut_sym", LUT3, 2, 1, false }, { "rle16_7symlut_sym", LUT7, 2, 1, false },
  { "rle16_byte", PLAIN, 2, 0, false }, { "rle16_byte_packed", PACKED, 2, 0, false }, { "rle16_3symlut_byte", LUT3, 2, 0, false }, { "rle16_7symlut_byte", LUT7, 2, 0, false },
  { "rle24_sym", PLAIN, 3, 1, false }, { "rle24_sym_packed", PACKED, 3, 1, false }, { "rle24_3symlut_sym", LUT3, 3, 1, false }, { "rle24_7symlut_sym", LUT7, 3, 1, false },
  { "rle24_byte", PLAIN, 3, 0, false }, { "rle24_byte_packed", PACKED, 3, 0, false }, { "rle24_3symlut_byte", LUT3, 3, 0, false }, { "rle24_7symlut_byte", LUT7, 3, 0, false },
  { "rle32_sym", PLAIN, 4, 1, false }, { "rle32_sym_packed", PACKED, 4, 1, false }, { "rle32_3symlut_sym", LUT3, 4, 1, false }, { "rle32_7symlut_sym", LUT7, 4, 1, false },
  { "rle32_byte", PLAIN, 4, 0, false }, { "rle32_byte_packed", PACKED, 4, 0, false }, { "rle32_3symlut_byte", LUT3, 4, 0, false }, { "rle32_7symlut_byte", LUT7, 4, 0, false },
  { "rle48_sym", PLAIN, 6, 1, false }, { "rle48_sym_packed", PACKED, 6, 1, false }, { "rle48_3symlut_sym", LUT3, 6, 1, false }, { "rle48_7symlut_sym", LUT7, 6, 1, false },
  { "rle48_byte", PLAIN, 6, 0, false }, { "rle48_byte_packed", PACKED, 6, 0, false }, { "rle48_3symlut_byte", LUT3, 6, 0, false }, { "rle48_7symlut_byte", LUT7, 6, 0, false },
  { "rle64_sym", PLAIN, 8, 1, false }, { "rle64_sym_packed", PACKED, 8, 1, false }, { "rle64_3symlut_sym", LUT3, 8, 1, false }, { "rle64_7symlut_sym", LUT7, 8, 1, false },
  { "rle64_byte", PLAIN, 8, 0, false }, { "rle64_byte_packed", PACKED, 8, 0, false }, { "rle64_3symlut_byte", LUT3, 8, 0, false }, { "rle64_7symlut_byte", LUT7, 8, 0, false },
  // 128 bit symbols
  { "rle128_sym", PLAIN, 16, 1, false }, { "rle128_sym_packed", PACKED, 16, 1, false }, { "rle128_byte", PLAIN, 16, 0, false }, { "rle128_byte_packed", PACKED, 16, 0, false },
  // Short family (reference: src/rle.h:202-348, src/codec_funcs.h:283-388)
  { "rle8_multi_short", SHORT0, 1, 0, false }, { "rle8_1symlut_short", SHORT1, 1, 0, false }, { "rle8_3symlut_short", SHORT3, 1, 0, false }, { "rle8_7symlut_short", SHORT7, 1, 0, false },
  { "rle16_sym_short", SHORT0, 2, 1, false }, { "rle16_1symlut_sym_short", SHORT1, 2, 1, false }, { "rle16_3symlut_sym_short", SHORT3, 2, 1, false }, { "rle16_7symlut_sym_short", SHORT7, 2, 1, false },
  { "rle16_byte_short", SHORT0, 2, 0, false }, { "rle16_1symlut_byte_short", SHORT1, 2, 0, false }, { "rle16_3symlut_byte_short", SHORT3, 2, 0, false }, { "rle16_7symlut_byte_short", SHORT7, 2, 0, false },
  { "rle24_sym_short", SHORT0, 3, 1, false }, { "rle24_1symlut_sym_short", SHORT1, 3, 1, false }, { "rle24_3symlut_sym_short", SHORT3, 3, 1, false }, { "rle24_7symlut_sym_short", SHORT7, 3, 1, false },
  { "rle24_byte_short", SHORT0, 3, 0, false }, { "rle24_1symlut_byte_short", SHORT1, 3, 0, false }, { "rle24_3symlut_byte_short", SHORT3, 3, 0, false }, { "rle24_7symlut_byte_short", SHORT7, 3, 0, false },
  { "rle32_sym_short", SHORT0, 4, 1, false }, { "rle32_1symlut_sym_short", SHORT1, 4, 1, false }, { "rle32_3symlut_sym_short", SHORT3, 4, 1, false }, { "rle32_7symlut_sym_short", SHORT7, 4, 1, false },
  { "rle32_byte_short", SHORT0, 4, 0, false }, { "rle32_1symlut_byte_short", SHORT1, 4, 0, false }, { "rle32_3symlut_byte_short", SHORT3, 4, 0, false }, { "rle32_7symlut_byte_short", SHORT7, 4, 0, false },
  { "rle48_sym_short", SHORT0, 6, 1, false }, { "rle48_1symlut_sym_short", SHORT1, 6, 1, false }, { "rle48_3symlut_sym_short", SHORT3, 6, 1, false }, { "rle48_7symlut_sym_short", SHORT7, 6, 1, false },
  { "rle48_byte_short", SHORT0, 6, 0, false }, { "rle48_1symlut_byte_short", SHORT1, 6, 0, false }, { "rle48_3symlut_byte_short", SHORT3, 6, 0, false }, { "rle48_7symlut_byte_short", SHORT7, 6, 0, false },
  { "rle64_sym_short", SHORT0, 8, 1, false }, { "rle64_1symlut_sym_short", SHORT1, 8, 1, false }, { "rle64_3symlut_sym_short", SHORT3, 8, 1, false }, { "rle64_7symlut_sym_short", SHORT7, 8, 1, false },
  { "rle64_byte_short", SHORT0, 8, 0, false }, { "rle64_1symlut_byte_short", SHORT1, 8, 0, false }, { "rle64_3symlut_byte_short", SHORT3, 8, 0, false }, { "rle64_7symlut_byte_short", SHORT7, 8, 0, false },
  // Greedy encoders (reference: src/rle.h:398-416); the decode side is the Short decoder of the same grammar
  { "rle16_1symlut_byte_short_greedy", SHORT1, 2, 0, true }, { "rle16_3symlut_byte_short_greedy", SHORT3, 2, 0, true }, { "rle16_7symlut_byte_short_greedy", SHORT7, 2, 0, true },
  { "rle24_1symlut_byte_short_greedy", SHORT1, 3, 0, true }, { "rle24_3symlut_byte_short_greedy", SHORT3, 3, 0, true }, { "rle24_7symlut_byte_short_greedy", SHORT7, 3, 0, true },
  { "rle32_1symlut_byte_short_greedy", SHORT1, 4, 0, true }, { "rle32_3symlut_byte_short_greedy", SHORT3, 4, 0, true }, { "rle32_7symlut_byte_short_greedy", SHORT7, 4, 0, true },
  { "rle48_1symlut_byte_short_greedy", SHORT1, 6, 0, true }, { "rle48_3symlut_byte_short_greedy", SHORT3, 6, 0, true }, { "rle48_7symlut_byte_short_greedy", SHORT7, 6, 0, true },
  { "rle64_1symlut_byte_short_greedy", SHORT1, 8, 0, true }, { "rle64_3symlut_byte_short_greedy", SHORT3, 8, 0, true }, { "rle64_7symlut_byte_short_greedy", SHORT7, 8, 0, true },
  // one symbol per stream, none in the packets (src/rle.h:223-224)
  { "rle8_single_short", SHORT_SINGLE, 1, 0, false },
};

inline int codec_id_not_in_table() { return -1; }   // (not constexpr: to reach it in a constant expression is the compile error)
constexpr int codec_id(Family fam, int S, int aligned, bool greedy = false)
{
  for (int c = 0; c < kCodecCount; c++)
    if (kCodecs[c].fam == fam && kCodecs[c].S == S && kCodecs[c].aligned == aligned && kCodecs[c].greedy == greedy) return c;
  return codec_id_not_in_table();
}
constexpr int codec_id(int fam, int S, int aligned, bool greedy = false) { return codec_id((Family)fam, S, aligned, greedy); }   // (kernels take FAM as an int)

static_assert(kCodecCount == HSRLE_CODEC_COUNT, "one row per public codec id");
static_assert(codec_id(PLAIN, 1, 0) == HSRLE_RLE8_MULTI && codec_id(PACKED, 1, 0) == HSRLE_RLE8_PACKED_MULTI && codec_id(LUT3, 1, 0) == HSRLE_RLE8_3SYMLUT &&
              codec_id(LUT7, 1, 0) == HSRLE_RLE8_7SYMLUT && codec_id(SINGLE, 1, 0) == HSRLE_RLE8_SINGLE && codec_id(PACKED_SINGLE, 1, 0) == HSRLE_RLE8_PACKED_SINGLE, "8 bit ids");
static_assert(codec_id(PLAIN, 2, 1) == HSRLE_RLE16_SYM && codec_id(PLAIN, 3, 1) == HSRLE_RLE24_SYM && codec_id(PLAIN, 4, 1) == HSRLE_RLE32_SYM && codec_id(PLAIN, 6, 1) == HSRLE_RLE48_SYM &&
              codec_id(PLAIN, 8, 1) == HSRLE_RLE64_SYM && codec_id(PACKED, 2, 0) == HSRLE_RLE16_BYTE_PACKED && codec_id(LUT3, 4, 1) == HSRLE_RLE32_3SYMLUT_SYM &&
              codec_id(LUT7, 8, 0) == HSRLE_RLE64_7SYMLUT_BYTE, "2 .. 8 byte symbol ids");
static_assert(codec_id(PLAIN, 16, 1) == HSRLE_RLE128_SYM && codec_id(PACKED, 16, 1) == HSRLE_RLE128_SYM_PACKED && codec_id(PLAIN, 16, 0) == HSRLE_RLE128_BYTE &&
              codec_id(PACKED, 16, 0) == HSRLE_RLE128_BYTE_PACKED, "128 bit ids");
static_assert(codec_id(SHORT0, 1, 0) == HSRLE_RLE8_MULTI_SHORT && codec_id(SHORT1, 1, 0) == HSRLE_RLE8_1SYMLUT_SHORT && codec_id(SHORT3, 1, 0) == HSRLE_RLE8_3SYMLUT_SHORT &&
              codec_id(SHORT7, 1, 0) == HSRLE_RLE8_7SYMLUT_SHORT && codec_id(SHORT0, 2, 1) == HSRLE_RLE16_SYM_SHORT && codec_id(SHORT0, 3, 1) == HSRLE_RLE24_SYM_SHORT &&
              codec_id(SHORT0, 4, 1) == HSRLE_RLE32_SYM_SHORT && codec_id(SHORT0, 6, 1) == HSRLE_RLE48_SYM_SHORT && codec_id(SHORT0, 8, 1) == HSRLE_RLE64_SYM_SHORT &&
              codec_id(SHORT_SINGLE, 1, 0) == HSRLE_RLE8_SINGLE_SHORT, "Short family ids");
static_assert(codec_id(SHORT1, 2, 0, true) == HSRLE_RLE16_1SYMLUT_BYTE_SHORT_GREEDY && codec_id(SHORT1, 3, 0, true) == HSRLE_RLE24_1SYMLUT_BYTE_SHORT_GREEDY &&
              codec_id(SHORT1, 4, 0, true) == HSRLE_RLE32_1SYMLUT_BYTE_SHORT_GREEDY && codec_id(SHORT1, 6, 0, true) == HSRLE_RLE48_1SYMLUT_BYTE_SHORT_GREEDY &&
              codec_id(SHORT1, 8, 0, true) == HSRLE_RLE64_1SYMLUT_BYTE_SHORT_GREEDY, "Greedy ids");

// ---- what the host code asks of a row ----
constexpr bool is_single(const CodecInfo &c) { return c.fam == SINGLE || c.fam == PACKED_SINGLE || c.fam == SHORT_SINGLE; }   // ONE symbol per stream / block: picked first, its byte follows the header
constexpr bool is_greedy(const CodecInfo &c) { return c.greedy; }
constexpr bool is_short(const CodecInfo &c) { return c.fam >= SHORT0; }
constexpr bool is_lut_header(const CodecInfo &c) { return c.fam == LUT3 || c.fam == LUT7 || is_short(c); }   // 8-byte stream header
// list length K of the move-to-front list: 0 / 1 / 3 / 7 (hsrle_common.hip.h: Traits::K)
constexpr int list_len(const CodecInfo &c) { return (c.fam == LUT3 || c.fam == SHORT3) ? 3 : ((c.fam == LUT7 || c.fam == SHORT7) ? 7 : (c.fam == SHORT1 ? 1 : 0)); }
// symbol-state slots of the codec's decoder (IndexState<FAM>::KE): 0 plain / Single / 0-symbol Short, 1 Packed / 1-symbol list, 3, 7
constexpr int state_slots(const CodecInfo &c) { return (c.fam == PACKED || c.fam == PACKED_SINGLE) ? 1 : list_len(c); }
// 9 bytes (a mode byte behind the two sizes) for the 8 bit plain / Packed / Single codecs, 8 elsewhere (Traits::kHeaderSize)
constexpr uint32_t header_size(const CodecInfo &c) { return (c.S == 1 && !is_lut_header(c)) ? 9u : 8u; }
// the 7-bit-or-4-byte range field: Packed byte-aligned and 8 bit Packed; sym-aligned Packed is the hybrid (Traits::kRange7)
constexpr bool range7(const CodecInfo &c) { return c.fam == PACKED && !c.aligned; }
// the run length every state of the codec's encoder stores (SURVEY.md A.2 LONG / the Short family's SMINL): the monolithic and the split encode cut behind such runs
constexpr uint32_t cut_long(const CodecInfo &c)
{
  const uint32_t S = c.S;
  // Greedy encoders (rleX_Xsl_short.h:746-1000): a run of SMINL = S + 11 bytes is stored whatever the state -- but the scan may enter a
  // periodic stretch up to ~2 S bytes late (through a prefix of a listed symbol), so a stretch is a cut from S + 11 + 3 S bytes on
  if (c.greedy) return 4u * S + 11u;
  switch (c.fam)
  {
  case SHORT_SINGLE: return 27u;                                  // rle8_single_short: runs of THE symbol of SMINL = 11 bytes are always stored; + 16, the body counts a run from where its search found it
  case SINGLE: return 8u;                                         // 8 bit Single: runs of THE symbol with count >= LONG (rle8_extreme_cpu.h:10-11, :21-23)
  case PACKED_SINGLE: return 10u;
  case PLAIN: return S == 1 ? 6u : S + 11u;                       // rle8_extreme_cpu.h:974: count >= 6 whatever the range; rleX_extreme_cpu.h:10-11, rle128_extreme_cpu.h:10-11
  case PACKED: return S == 1 ? 11u : (c.aligned ? S + 10u : S + 11u);   // rle8_extreme_cpu.h:978 (body) and :122 (tail); sym-aligned Packed: the hybrid of A.5 q10
  case LUT3: case LUT7: return S + 10u;                           // rleX_Xsl.h:132
  case SHORT0: return S + 12u;                                    // rleX_Xsl_short.h: always stored from S + 12 on (0-symbol codec)
  default: return S + 11u;                                        // ... from S + 11 on with a list of 1 / 3 / 7 symbols
  }
}
// the codecs whose encoder state at a cut is fixed by the cut itself (no list, or a one-symbol list = the cut's symbol): plain / Packed / Short without or with a
// one-symbol list, of 1 .. 8 byte symbols -- the chunks of their monolithic streams go to the windowed position-parallel encoders
constexpr bool chunk_mode(const CodecInfo &c) { return (c.fam == PLAIN || c.fam == PACKED || c.fam == SHORT0 || c.fam == SHORT1) && c.S <= 8 && !c.greedy; }
// windowed encoders, blocks of ANY size: plain / Packed of 1 .. 8 byte symbols write 8 or 32 bit fields whatever the block size (encode_choice)
constexpr bool any_block_windowed(const CodecInfo &c) { return (c.fam == PLAIN || c.fam == PACKED) && c.S <= 8; }
// Greedy with a list of ONE symbol: behind a stored run the list is that run's symbol, so a chunk's first guess is right (encode_choice: the split encode)
constexpr bool greedy_one_symbol_list(const CodecInfo &c) { return c.greedy && c.fam == SHORT1; }
// the codecs that have a many-lane chunk encoder but no run list encoder: small containers of 1 .. 4 KiB blocks take the split encode IF the
// caller's workspace has its regions (hsrle_compress_workspace_size_codec; the library's own scratch always has)
constexpr bool split_small(const CodecInfo &c) { return is_single(c) || c.S == 16 || greedy_one_symbol_list(c); }
// Plain block decode: the ratio (payload + tail pad) / uncompressed size, in thousandths, below which a container takes the decoder instantiation with the
// 64-byte stream ring (hsrle_launch.h: decode_ring_small says why and when); 0 = the codec has no such instantiation.  THE statement of these thresholds.
// 1 / 2 byte symbols: 250 -- rle16_sym at 0.23 still gains 6 %.  3 / 4 byte symbols: 215 (round 4; 200 before: rle32_3symlut_sym video-shaped at 0.2042 gains
// 9 % with the small ring) -- 8 GiB video-shaped rle32_3symlut_byte (0.17) +16 %, rle24_7symlut_byte_short (0.19) +12 %, every 24 / 32 bit row of the sweep
// below 0.2 gains 10 - 20 %, but rle24_sym (0.26) -3 %, rle32_sym (0.30) -8 %.  6 / 8 / 16 byte symbols: never (their packets are large: below a ratio of 0.2
// the 64-byte ring cost the 7-symbol LUT codecs 24 % on run-distributed data, 19 % on video-shaped; sweep of 8 GiB buffers).
constexpr uint32_t small_ring_per_mille(const CodecInfo &c) { return c.S <= 2 ? 250u : (c.S <= 4 ? 215u : 0u); }

// ---- block decode: which k_decode_blocks instantiation a launch takes.  THE rule; hsrle_launch.h: launch_decode_codec instantiates what it can return ----
struct DecodeKnobs   // A/B builds (hsrle_launch.h: kDecodeKnobs); the shipped library has none set
{
  bool alwaysEnt = false;   // HSRLE_DECODE_ALWAYS_ENT: 3 .. 8 byte symbols keep the entry-record prologue (and with it the 128-byte ring) for plain containers too
  bool pe8 = false;         // HSRLE_DEC8_PE: plain containers of rle8_multi / rle8_packed_multi go to parse + expand (csrc/experiments/hsrle_decode8pe.hip.h)
};
// The order of the three sections of a trip of the 8 bit packet loop (hsrle_decode.hip.h, `S == 1`): false = header, literals, run (H L R); true = literals, run,
// header (L R H: no header section in the first trip of a pass -- a lane parses at the end of the trip that finished its packet).  Part of the rule: the kernel
// asks with its family and SGL.  Same-box A/B per row (profiles/r11_decode_loop_order.md, 2 GiB, run-distributed / video-shaped): the list kernels gain with L R H
// (rle8_3symlut +3.7 / +1.9 %, rle8_7symlut +6.0 / +2.4 %, rle8_3symlut_short +4.2 / +4.3 %, rle8_7symlut_short +3.8 / +5.0 %) and so does the Packed multi kernel
// (the headline: -1.3 % time; at 2 GiB -0.1 / +0.9 %); the plain multi kernel (rle8_multi +0.6 / -1.1 %) and the kernels of the Single ids (rle8_packed_single
// 0 / -0.9 %) lose on video-shaped data more than the spread between two batches of one library, and with them every kernel that was not measured keeps H L R.
// A/B builds: -DHSRLE_DEC8_LRH=0 / 1 forces one order on every 8 bit kernel.
constexpr bool dec8_loop_lrh(Family fam, bool sgl)
{
#ifdef HSRLE_DEC8_LRH
  return HSRLE_DEC8_LRH != 0;
#else
  return fam == LUT3 || fam == LUT7 || fam == SHORT3 || fam == SHORT7 || (fam == PACKED && !sgl);
#endif
}

// Lazy run fill (hsrle_decode.hip.h, `S == 1`, uncapped rounds without an output window: the kernels with the full-row flush): the R section stores only the first
// chunk of what it fills and marks the chunks that lie wholly inside the run behind it in a per-row bit mask; the full-row flush's serving lane reads the stored chunk
// in front of a marked one instead and broadcasts its last byte.  Part of the rule like the section order above: the kernel asks with its family, SGL and ring, and every
// kernel that was not measured keeps the stores.  Same-box A/B per row (profiles/r14_decode_run_fill.md, 2 GiB, run-distributed / video-shaped, against the spread
// between two batches of the parent): the Packed multi kernel (the headline: -1.7 % time at 8 GiB; rle8_packed_multi +1.7 / +1.6 %), the plain multi kernel (rle8_multi
// +1.0 / +2.5 %) and the 3-symbol list kernel (rle8_3symlut +1.8 / +1.2 %) gain on both shapes and take it.  The kernels of the Single ids lose on run data
// (rle8_single -0.8 %, rle8_packed_single -0.7 % / +4.2 %, rle8_single_short -0.6 / -0.2 %), the Short kernels without and with a one-symbol list gain on run data only
// (+3.2 / +0.1 %, +4.0 / 0.0 %), and the 7-symbol list kernel would lose a wave per SIMD (164 -> 170 VGPRs): they keep the stores.  So do the instantiations with the
// 64-byte stream ring: those rows ran the 128-byte ring, nobody measured the small one, and the 64 mask bytes would be its eleventh LDS allocation granule of 1 280 bytes
// (12 800 bytes are exactly ten: 12 waves per CU, which is also what the registers allow; eleven granules hold 11).
// A/B builds: -DHSRLE_DEC8_LAZY=0 / 1 forces it on every 8 bit kernel that can take it, either ring.
constexpr bool dec8_lazy_fill(Family fam, bool sgl, int ring)
{
#ifdef HSRLE_DEC8_LAZY
  return HSRLE_DEC8_LAZY != 0;
#else
  return ring == 128 && (((fam == PACKED || fam == PLAIN) && !sgl) || fam == LUT3);
#endif
}

struct DecodeVariant
{
  Family fam;          // the kernel's FAM: Single ids decode with the multi kernels' general form, Greedy ids with the Short decoder of their grammar (the row's family)
  bool sgl, ent, win;  // k_decode_blocks SGL / ENT / WIN
  int ring;            // stream ring: 64, or 128 = the default one (kDecodeRing / kDec8Ring)
  bool list8;          // an 8 bit plain / Packed kernel: tile, step and ring are kDec8Tile / kDec8Step / kDec8Ring
  bool pe;             // not k_decode_blocks at all: k_decode8_pe<fam> (DecodeKnobs::pe8)
};
// window: the launch has an output window (range decode); entries: lanes start from entry records; smallRing: decode_ring_small() said yes
constexpr DecodeVariant decode_variant(const CodecInfo &c, bool window, bool entries, bool smallRing, DecodeKnobs k = DecodeKnobs{})
{
  const Family fam = c.fam == SINGLE ? PLAIN : (c.fam == PACKED_SINGLE ? PACKED : c.fam);
  const bool list8 = c.S == 1 && (fam == PLAIN || fam == PACKED);
  const bool sgl = !(c.S == 1 && (c.fam == PLAIN || c.fam == PACKED));   // rle8_multi / rle8_packed_multi: their encoders only write mode 0
  if (window) return { fam, sgl, true, true, 128, list8, false };
  const bool small = !entries && smallRing && small_ring_per_mille(c) != 0u;   // (blocks decoded from entry records keep the 128-byte ring)
  if (c.S == 1)   // one byte symbols: one instantiation with the record prologue serves both
    return (k.pe8 && !sgl) ? DecodeVariant{ fam, sgl, true, false, 128, list8, !entries } : DecodeVariant{ fam, sgl, true, false, small ? 64 : 128, list8, false };
  // wider symbols: plain containers take the instantiation without the entry-record prologue (same-box A/B on run-distributed data:
  // rle32_3symlut_byte +6 %, rle48_7symlut_sym +4 %, rle64_sym +-0; the 128 bit codecs +10 %)
  if (entries || (k.alwaysEnt && c.S >= 3 && c.S <= 8)) return { fam, true, true, false, 128, false, false };
  return { fam, true, false, false, small ? 64 : 128, false, false };
}

// ---- container encode: which encoder takes a container, and which workspace regions it needs.  THE rule (DESIGN.md 4.2 has it as a table); compress_async,
// hsrle_encode_path and hsrle_compress_workspace_size_codec all ask it (hsrle_capi_container.h: encode_choice_of) ----
constexpr uint32_t kEncodeWaveBytes = 4096u;        // what a wave of the position-parallel encoders holds (= kPpMaxBlock = kPpwWindow: hsrle_capi_container.h asserts it)
constexpr uint32_t kSplitEncodeBelow = 131072u;     // blocks: from here on one lane per block fills the device -- no split encode, no run list
constexpr uint32_t kSplitPieces = 4u, kSplitPiecesMax = 8u;   // cut finder lanes per block of the split encode (the workspace is planned for the larger number: split_pieces())
// (the plain / Packed codecs write 8 or 32 bit fields whatever the block size; the LUT / Short forms choose their field widths -- and the reference its penalties, with
//  thresholds of 0xFFFFF: rleX_Xsl.h:130, rleX_Xsl_short.h:178 -- by the values: below 1 MiB per block no count or range gets there and "every run is stored" holds)
constexpr uint32_t kPpwListMaxBlock = (1u << 20) - 128u;
// The bound the block encoders of the list codecs rest on: the largest range of a block is its size + 2, the largest stored count below that.  Who leaves the 20 bit
// term out because of it: hsrle_encodeSp.hip.h (ppS_decide<.., WIDE = false>) and hsrle_encodeLp / Lpw.hip.h (stored_with).  hsrle_encodeSpw.hip.h instantiates
// ppS_decide<.., WIDE = true> for all its kernels: its CHUNK mode (chunk_mode() above) has no such bound and needs the term; in its block mode the term is compiled in
// and, by this bound, never taken.
static_assert(kEncodeWaveBytes + 2u <= 0xFFFFFu && kPpwListMaxBlock + 2u <= 0xFFFFFu, "blocks of the list codecs' position-parallel encoders must stay below the reference's 20 bit penalty step");

enum PpwKind : int { PPW_NONE = 0, PPW_8, PPW_L, PPW_S };   // which windowed launcher a row has (CodecLaunch::ppw8, then ppwL, then ppwS)
// what a row of the launch table has; the host fills it from g_launch[codec] (wenc: experiment builds, the wave encoder of rle8_multi / rle8_packed_multi)
struct EncodeCaps { bool pp; PpwKind ppw; bool menc, enc; bool wenc = false; };
// the split encode's regions in a workspace (2 - 3 x the input): none, those of blocks above 4 KiB (every workspace sized without a codec has them), or those of the
// split_small() codecs' blocks of 1 .. 4 KiB too (the library's own scratch, a workspace of hsrle_compress_workspace_size_codec)
enum SplitRegions : int { SPLIT_NONE = 0, SPLIT_LARGE = 1, SPLIT_ALL = 2 };
struct EncodeKnobs   // experiment builds (hsrle_capi_container.h: encode_knobs); the shipped library passes the defaults
{
  uint32_t pp = 0u;             // HSRLE_PP: 1 = the position-parallel encoders always, 2 = never
  uint32_t runList = 0u;        // HSRLE_RUNLIST: 1 = the run list encoders always, 2 = never
  uint32_t waveMaxBlock = 0u;   // HSRLE_ENCODE_WAVE=1: blocks up to this size go to the wave encoder (0: off)
  uint32_t ppwMinBlocks = 1u;   // -DHSRLE_PPW_MIN_BLOCKS (0xFFFFFFFF = never windowed)
  uint32_t chunkBlocks = 0u;    // HSRLE_ENCODE_CHUNK_BLOCKS: the ring encoders take the container in chunks of so many blocks (0: in one piece)
  SplitRegions generic = SPLIT_LARGE;   // what a workspace sized without a codec reserves (experiment builds: SPLIT_ALL, so that HSRLE_RUNLIST=2 can send small blocks to the split encode)
};
enum EncodePath : int { ENC_UNSUPPORTED = 0, ENC_WAVE, ENC_PP, ENC_PPW, ENC_SPLIT, ENC_RING_CHUNKS, ENC_RING };
// ppw: the windowed launcher of ENC_PPW; runList: ENC_RING's launcher hands the container to the run list encoder (hsrle_encode8r.hip.h); regions: what the path's workspace is planned with
struct EncodeChoice { EncodePath path; PpwKind ppw; bool runList; SplitRegions regions; };
// blocks per chunk of the ring encoders (EncodeKnobs::chunkBlocks; else the whole container).  No short last chunk: up to 1.5 chunks go in one piece
constexpr uint64_t encode_chunk(uint64_t nBlocks, EncodeKnobs k)
{
  const uint64_t chunk = k.chunkBlocks ? k.chunkBlocks : 0xFFFFFFF0ull;
  return nBlocks < chunk + chunk / 2u ? nBlocks : chunk;
}

// which containers the run list encoder takes (hsrle_encode8r.hip.h; the ring launchers of inst_w8.hip ask too; force: 1 always, 2 never -- experiment builds)
constexpr bool run_list_applies(uint64_t nBlocks, uint32_t B, uint64_t U, uint32_t force = 0u)
{
  return B >= 1024u && B <= kEncodeWaveBytes && U >= 1024u && force != 2u && (force == 1u || nBlocks < kSplitEncodeBelow);
}
// (round 6: the codecs with a position-parallel encoder have no run list instantiation any more; before, all but Single, 128 bit and Greedy had one)
constexpr bool run_list_codec(const CodecInfo &c, EncodeCaps caps) { return !is_single(c) && c.S != 16 && !c.greedy && !caps.pp; }

// have: the split regions of the workspace at hand.  noSplit: the second attempt of hsrle_compress_dev, after the split encode struck its own container.
constexpr EncodeChoice encode_choice(const CodecInfo &c, EncodeCaps caps, uint64_t U, uint32_t B, uint64_t nBlocks, SplitRegions have, bool noSplit, EncodeKnobs k = EncodeKnobs{})
{
  const bool onePiece = nBlocks <= encode_chunk(nBlocks, k);
  const bool small = B <= kEncodeWaveBytes;
  // position-parallel: a block per wave, whatever the container's size (faster than the ring and the run list encoders from 1 MiB to 8 GiB: experiments/r05, call 20); above
  // 4 KiB window by window -- the list codecs below 1 MiB per block only, and the windows are counted in 32 bits (16 TiB)
  const bool ppOn = k.pp != 2u, pp = caps.pp && small && ppOn;
  const bool ppw = caps.ppw != PPW_NONE && !small && ppOn && (any_block_windowed(c) || B <= kPpwListMaxBlock) && nBlocks * ((B + kEncodeWaveBytes - 1u) / kEncodeWaveBytes) <= 0xFFFFFFF0ull &&
                   (k.pp == 1u || nBlocks >= k.ppwMinBlocks);
  // noSplit suppresses only the upgrade to the small-block regions: a workspace planned without a codec keeps its split path (ADVICE r6 item 1 -- to fix it, let noSplit give SPLIT_NONE here)
  const SplitRegions has = (noSplit && have == SPLIT_ALL) ? k.generic : have;
  // (a windowed codec's workspace is planned without the regions; up to 4 KiB they serve the codecs that have no run list encoder)
  const bool regionsHere = !ppw && (small ? has == SPLIT_ALL && (split_small(c) || k.generic == SPLIT_ALL) : has != SPLIT_NONE);
  const bool runList = run_list_codec(c, caps) && run_list_applies(nBlocks, B, U, k.runList);
  // split encode: the codecs with a chunk encoder (the ring encoders' chunk mode; 8 bit Single and 128 bit: the per-lane chunk encoders of the monolithic path), unless the run
  // list encoders take the container whole.  Greedy: the lists of 3 / 7 symbols decide which runs the scan stores, so a chunk's list is only known when the chunk in front of it
  // is final -- measured (88 MB frame, rle32_7symlut: two full passes + three repair rounds 3.7 ms against 3.1 ms with one lane per block); a list of ONE symbol behind a stored
  // run is that run's symbol, and the first guess is right.  Single: the per-block symbol pick holds a block in LDS (hsrle_encode8s.hip.h).
  const bool split = regionsHere && caps.menc && !(run_list_codec(c, caps) && run_list_applies(nBlocks, B, 1024u, k.runList)) && nBlocks < kSplitEncodeBelow && B >= 1024u && B <= (1u << 20) &&
                     B % (kSplitPieces * 128u) == 0u && !(c.greedy && !greedy_one_symbol_list(c)) && !(is_single(c) && B > 32768u);
  const EncodePath path = !caps.enc ? ENC_UNSUPPORTED : (caps.wenc && B <= k.waveMaxBlock) ? ENC_WAVE                                 // (in chunks: the ring encoders only)
                        : (onePiece && pp) ? ENC_PP : (onePiece && ppw) ? ENC_PPW : (onePiece && split) ? ENC_SPLIT : !onePiece ? ENC_RING_CHUNKS : ENC_RING;
  const SplitRegions regions = ppw ? SPLIT_NONE : ((path == ENC_SPLIT && small) ? SPLIT_ALL : k.generic);
  return { path, path == ENC_PPW ? caps.ppw : PPW_NONE, path == ENC_RING && runList, regions };
}

// ---- container decode: the argument checks of every decode entry point (hsrle_capi_container.h: decode_prologue), in their observable order; no device is asked ----
constexpr bool valid_block_size(uint32_t B) { return B >= HSRLE_MIN_BLOCK_SIZE && B <= HSRLE_MAX_BLOCK_SIZE && (B % 128u) == 0; }
constexpr uint64_t block_count(uint64_t U, uint32_t B) { return (U + B - 1) / B; }
// a null pointer beats an info that does not describe a container ...
constexpr int decode_info_check(const void *dContainer, const hsrle_container_info_t *info, const void *dOut)
{
  if (dContainer == nullptr || info == nullptr || dOut == nullptr) return HSRLE_ERR_ARGUMENT;
  const bool ok = info->codec < (uint32_t)kCodecCount && valid_block_size(info->blockSize) && info->blockCount == block_count(info->uncompressedSize, info->blockSize);
  return ok ? HSRLE_OK : HSRLE_ERR_FORMAT;
}
// ... which beats a block range outside it, which beats an output buffer that does not hold the whole container
constexpr int decode_range_check(const hsrle_container_info_t &info, uint32_t first, uint32_t count, uint64_t cap)
{
  return (uint64_t)first + count > info.blockCount ? HSRLE_ERR_ARGUMENT : (cap < info.uncompressedSize ? HSRLE_ERR_CAPACITY : HSRLE_OK);
}

} // namespace hsrle
