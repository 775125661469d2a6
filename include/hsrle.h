/*
 * hsrle.h -- C ABI of libhsrle_hip.so: the MI355X-native implementation of the hypersonic-rle-kit
 * `rleX_extreme` encode / decode hot path (8/16/24/32/48/64/128 bit symbols; plain, Packed, 3/7 symbol LUT
 * and Single variants).
 *
 * Three layers, all `extern "C"`, plain pointers and sizes:
 *
 *  1. DROP-IN entry points with exactly the names, signatures and error behaviour of the reference's public
 *     header (reference: src/rle.h:100-394; registered in src/codec_funcs.h:270-410).  Host pointers in, host
 *     pointers out, one monolithic reference stream.  A maintainer links libhsrle_hip.so instead of
 *     rle8_extreme_cpu.c / rleX_extreme_cpu.c / rle{24,48,128}_extreme_cpu.c / rleX_Xsl.c (INTEGRATION.md has the link recipe;
 *     the reference's own `hsrlekit` built that way passes its `--test` run on the GPU, tests/test_gpu_parity.py).
 *
 *  2. Device-resident block API (`hsrle_*_dev`): the input is cut into fixed-size blocks, every block is encoded
 *     as an independent, self-terminating reference stream (bit-exact with what the reference encoder produces
 *     for that block) and the streams are concatenated behind an offset table.  This is the throughput path; its
 *     layout follows the reference's own sub-section container for rle8m
 *     (reference: src/rle8_low_entropy_cpu.c:131-250).
 *
 *  3. Host convenience wrappers around 2 (`hsrle_compress_host`, `hsrle_decompress_host`).
 *
 *  4. Multi-GPU: one container from the containers of W ranks and back, over RCCL (section 4 below).
 *
 * Threads and streams.  The device-pointer functions (2, 4, hsrle_decompress_mono_dev) keep NO library-owned state between calls: they
 * work on the caller's buffers, and what they need beyond those (the compression workspace when dWorkspace is NULL, status words) is
 * allocated stream-ordered on the caller's stream for the duration of the call.  Any number of threads may call them at the same time,
 * on the same or on different streams and devices (the device is the calling thread's current HIP device).  The host-pointer drop-in
 * functions (1, 3) stage through per-device buffers and hold that device's lock for the whole call: they are safe to call from several
 * threads, and calls on one device run one after the other (the reference's own callers are single threaded: src/main.c, src/rle_fuzz.c).
 * Device state is created lazily on first use (like the reference's rle8m_opencl_decompress does, src/rle8_ocl.c:324).  The library never
 * falls back to a CPU codec: if no HIP device is usable every entry point fails (drop-in functions return 0, hsrle_* an error code).
 */
#ifndef HSRLE_H
#define HSRLE_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------------------- */
/* codec ids.  One per (compress, decompress) pair of the reference's table that belongs to the hot path.      */

typedef enum hsrle_codec
{
  /* ids 0 / 1 name the multi-symbol ENCODERS: the blocks of such a container are mode-0 streams (what those encoders write); a     */
  /* Single-mode block in it is reported as a format error.  The drop-in rle8_decompress / rle8_packed_decompress take either mode. */
  HSRLE_RLE8_MULTI = 0,          /* rle8_multi_compress / rle8_decompress                     rle.h:101,103 */
  HSRLE_RLE8_PACKED_MULTI = 1,   /* rle8_packed_multi_compress / rle8_packed_decompress       rle.h:173,175 */
  HSRLE_RLE8_3SYMLUT = 2,        /* rle8_3symlut_*                                            rle.h:199-200 */
  HSRLE_RLE8_7SYMLUT = 3,        /* rle8_7symlut_*                                            rle.h:207-208 */
  HSRLE_RLE8_SINGLE = 4,         /* rle8_single_compress / rle8_decompress                    rle.h:102,103 */
  HSRLE_RLE8_PACKED_SINGLE = 5,  /* rle8_packed_single_compress / rle8_packed_decompress      rle.h:174,175 */

  /* for W in 16,24,32,48,64:  base = 6 + 8 * index(W);  base + k with k = */
  /*   0 sym  1 sym_packed  2 3symlut_sym  3 7symlut_sym  4 byte  5 byte_packed  6 3symlut_byte  7 7symlut_byte */
  HSRLE_RLE16_SYM = 6, HSRLE_RLE16_SYM_PACKED, HSRLE_RLE16_3SYMLUT_SYM, HSRLE_RLE16_7SYMLUT_SYM,
  HSRLE_RLE16_BYTE, HSRLE_RLE16_BYTE_PACKED, HSRLE_RLE16_3SYMLUT_BYTE, HSRLE_RLE16_7SYMLUT_BYTE,
  HSRLE_RLE24_SYM = 14, HSRLE_RLE24_SYM_PACKED, HSRLE_RLE24_3SYMLUT_SYM, HSRLE_RLE24_7SYMLUT_SYM,
  HSRLE_RLE24_BYTE, HSRLE_RLE24_BYTE_PACKED, HSRLE_RLE24_3SYMLUT_BYTE, HSRLE_RLE24_7SYMLUT_BYTE,
  HSRLE_RLE32_SYM = 22, HSRLE_RLE32_SYM_PACKED, HSRLE_RLE32_3SYMLUT_SYM, HSRLE_RLE32_7SYMLUT_SYM,
  HSRLE_RLE32_BYTE, HSRLE_RLE32_BYTE_PACKED, HSRLE_RLE32_3SYMLUT_BYTE, HSRLE_RLE32_7SYMLUT_BYTE,
  HSRLE_RLE48_SYM = 30, HSRLE_RLE48_SYM_PACKED, HSRLE_RLE48_3SYMLUT_SYM, HSRLE_RLE48_7SYMLUT_SYM,
  HSRLE_RLE48_BYTE, HSRLE_RLE48_BYTE_PACKED, HSRLE_RLE48_3SYMLUT_BYTE, HSRLE_RLE48_7SYMLUT_BYTE,
  HSRLE_RLE64_SYM = 38, HSRLE_RLE64_SYM_PACKED, HSRLE_RLE64_3SYMLUT_SYM, HSRLE_RLE64_7SYMLUT_SYM,
  HSRLE_RLE64_BYTE, HSRLE_RLE64_BYTE_PACKED, HSRLE_RLE64_3SYMLUT_BYTE, HSRLE_RLE64_7SYMLUT_BYTE,

  HSRLE_RLE128_SYM = 46,         /* rle128_sym_*          rle.h:124-125 */
  HSRLE_RLE128_SYM_PACKED = 47,  /* rle128_sym_packed_*   rle.h:146-147 */
  HSRLE_RLE128_BYTE = 48,        /* rle128_byte_*         rle.h:168-169 */
  HSRLE_RLE128_BYTE_PACKED = 49, /* rle128_byte_packed_*  rle.h:194-195 */

  /* Short family: one-byte packed headers with a 0 / 1 / 3 / 7 symbol move-to-front list.                 */
  HSRLE_RLE8_MULTI_SHORT = 50,   /* rle8_multi_short_*     rle.h:221-222 */
  HSRLE_RLE8_1SYMLUT_SHORT = 51, /* rle8_1symlut_short_*   rle.h:216-217 */
  HSRLE_RLE8_3SYMLUT_SHORT = 52, /* rle8_3symlut_short_*   rle.h:202-203 */
  HSRLE_RLE8_7SYMLUT_SHORT = 53, /* rle8_7symlut_short_*   rle.h:210-211 */
  /* for W in 16,24,32,48,64:  base = 54 + 8 * index(W);  base + k with k =                                              */
  /*   0 sym_short  1 1symlut_sym_short  2 3symlut_sym_short  3 7symlut_sym_short                                        */
  /*   4 byte_short 5 1symlut_byte_short 6 3symlut_byte_short 7 7symlut_byte_short            rle.h:228-348              */
  HSRLE_RLE16_SYM_SHORT = 54, HSRLE_RLE24_SYM_SHORT = 62, HSRLE_RLE32_SYM_SHORT = 70, HSRLE_RLE48_SYM_SHORT = 78, HSRLE_RLE64_SYM_SHORT = 86,

  /* Greedy encoders (rle.h:398-416): base = 94 + 3 * index(W) + {0 1symlut, 1 3symlut, 2 7symlut}; compress =                */
  /* rle{W}_{K}symlut_byte_short_compress_greedy, decompress = rle{W}_{K}symlut_byte_short_decompress (codec_funcs.h:298-388) */
  HSRLE_RLE16_1SYMLUT_BYTE_SHORT_GREEDY = 94, HSRLE_RLE24_1SYMLUT_BYTE_SHORT_GREEDY = 97, HSRLE_RLE32_1SYMLUT_BYTE_SHORT_GREEDY = 100,
  HSRLE_RLE48_1SYMLUT_BYTE_SHORT_GREEDY = 103, HSRLE_RLE64_1SYMLUT_BYTE_SHORT_GREEDY = 106,

  HSRLE_RLE8_SINGLE_SHORT = 109, /* rle8_single_short_*    rle.h:223-224 */

  HSRLE_CODEC_COUNT = 110
} hsrle_codec_t;

typedef enum hsrle_status
{
  HSRLE_OK = 0,
  HSRLE_ERR_ARGUMENT = 1,    /* NULL pointer, zero size, unknown codec, bad block size                       */
  HSRLE_ERR_CAPACITY = 2,    /* output / workspace buffer too small                                          */
  HSRLE_ERR_FORMAT = 3,      /* container or block stream header inconsistent / stream malformed             */
  HSRLE_ERR_DEVICE = 4,      /* no usable HIP device, or a HIP runtime call failed                           */
  HSRLE_ERR_UNSUPPORTED = 5  /* kernel for this codec is not available in this build                         */
} hsrle_status_t;

/* name <-> id, using the reference's naming ("rle8_packed_multi", "rle64_3symlut_byte", ...).  -1 if unknown. */
int hsrle_codec_from_name(const char *name);
const char *hsrle_codec_name(int codec);
const char *hsrle_status_string(int status);

/* ---------------------------------------------------------------------------------------------------------- */
/* 1. drop-in entry points (reference: src/rle.h).  0 = failure.                                               */

uint32_t rle_compress_bounds(const uint32_t inSize);   /* rle.h:100, rle8_extreme_cpu.c:22-28 */
uint32_t rle_decompress_additional_size(void);         /* rle.h:105, rle8_extreme_cpu.c:17-20 */

#define HSRLE_DECL_PAIR(name) \
  uint32_t name##_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize); \
  uint32_t name##_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
#define HSRLE_DECL_WIDTH(W) \
  HSRLE_DECL_PAIR(rle##W##_sym) HSRLE_DECL_PAIR(rle##W##_sym_packed) HSRLE_DECL_PAIR(rle##W##_byte) HSRLE_DECL_PAIR(rle##W##_byte_packed) \
  HSRLE_DECL_PAIR(rle##W##_3symlut_sym) HSRLE_DECL_PAIR(rle##W##_7symlut_sym) HSRLE_DECL_PAIR(rle##W##_3symlut_byte) HSRLE_DECL_PAIR(rle##W##_7symlut_byte)

/* 8 bit (irregular names; rle.h:101-103, :173-175, :199-200, :207-208) */
uint32_t rle8_multi_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_single_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_packed_multi_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_packed_single_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_packed_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
HSRLE_DECL_PAIR(rle8_3symlut)
HSRLE_DECL_PAIR(rle8_7symlut)

/* 16 / 24 / 32 / 48 / 64 bit (rle.h:107-122, :129-144, :151-166, :177-192, :250-258, :284-292, :318-326, :352-360, :386-394) */
HSRLE_DECL_WIDTH(16)
HSRLE_DECL_WIDTH(24)
HSRLE_DECL_WIDTH(32)
HSRLE_DECL_WIDTH(48)
HSRLE_DECL_WIDTH(64)

/* 128 bit (rle.h:124-125, :146-147, :168-169, :194-195) */
HSRLE_DECL_PAIR(rle128_sym)
HSRLE_DECL_PAIR(rle128_sym_packed)
HSRLE_DECL_PAIR(rle128_byte)
HSRLE_DECL_PAIR(rle128_byte_packed)

/* Short family: rle.h:202-203, :210-211, :216-217, :221-222 (8 bit), :228-348 (16..64 bit) */
#define HSRLE_DECL_SHORT_WIDTH(W) \
  HSRLE_DECL_PAIR(rle##W##_sym_short) HSRLE_DECL_PAIR(rle##W##_byte_short) HSRLE_DECL_PAIR(rle##W##_1symlut_sym_short) HSRLE_DECL_PAIR(rle##W##_1symlut_byte_short) \
  HSRLE_DECL_PAIR(rle##W##_3symlut_sym_short) HSRLE_DECL_PAIR(rle##W##_3symlut_byte_short) HSRLE_DECL_PAIR(rle##W##_7symlut_sym_short) HSRLE_DECL_PAIR(rle##W##_7symlut_byte_short)
HSRLE_DECL_PAIR(rle8_multi_short)
HSRLE_DECL_PAIR(rle8_single_short)
HSRLE_DECL_PAIR(rle8_1symlut_short)
HSRLE_DECL_PAIR(rle8_3symlut_short)
HSRLE_DECL_PAIR(rle8_7symlut_short)
HSRLE_DECL_SHORT_WIDTH(16)
HSRLE_DECL_SHORT_WIDTH(24)
HSRLE_DECL_SHORT_WIDTH(32)
HSRLE_DECL_SHORT_WIDTH(48)
HSRLE_DECL_SHORT_WIDTH(64)

/* Greedy encoders of the byte-aligned LUT Short codecs: rle.h:398-416 */
#define HSRLE_DECL_GREEDY(W) \
  uint32_t rle##W##_1symlut_byte_short_compress_greedy(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize); \
  uint32_t rle##W##_3symlut_byte_short_compress_greedy(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize); \
  uint32_t rle##W##_7symlut_byte_short_compress_greedy(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
HSRLE_DECL_GREEDY(16)
HSRLE_DECL_GREEDY(24)
HSRLE_DECL_GREEDY(32)
HSRLE_DECL_GREEDY(48)
HSRLE_DECL_GREEDY(64)
#undef HSRLE_DECL_GREEDY

#undef HSRLE_DECL_SHORT_WIDTH
#undef HSRLE_DECL_WIDTH
#undef HSRLE_DECL_PAIR

/* Generic form of the above (what the macro-declared functions forward to): one monolithic reference stream,
 * host pointers.  Mirrors `codecCallbacks[codec].compress_func / .decompress_func` (codec_funcs.h:262-266). */
uint32_t hsrle_compress_mono(int codec, const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize);
uint32_t hsrle_decompress_mono(int codec, const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize);

/*
 * Device-resident form of <codec>_decompress: ONE monolithic reference stream (what the reference's encoders and `hsrlekit` write:
 * src/main.c:835, :970; decoded there by src/rle8_extreme_cpu.h:702-764, src/rleX_extreme_cpu_decode.h:27-164, src/rleX_Xsl.h:1848-1881)
 * in device memory, decoded into device memory.  A stream has no random access, so the library first builds an entry-point index
 * (speculative packet walks per stream region, then a pass that PROVES the chain and repairs wrong guesses: csrc/hsrle_index.hip.h)
 * and then runs the block kernel from those entry points.  dStream must be 128-byte aligned and readable up to streamSize + 64.
 * dWorkspace >= hsrle_decompress_mono_workspace_size() bytes at any address (the library rounds it up to 16 bytes itself; the size includes that slack).  Synchronises `stream` (once, at the end, when every entry guess holds).  pStats (optional, host, 4 values): stream regions,
 * repair rounds, regions walked again, final look-back of the entry guess.  Returns HSRLE_OK, HSRLE_ERR_FORMAT (malformed stream / sizes do not match the header), ...
 */
uint64_t hsrle_decompress_mono_workspace_size(int codec, uint32_t uncompressedSize, uint32_t compressedSize);
/*
 * Device-resident form of <codec>_compress for the multi-symbol codecs of 8 to 64 bit symbols (plain, Packed, 3 / 7 symbol LUT and
 * the Short family; not Single, 128 bit, Greedy): ONE monolithic reference stream, byte-identical with the reference encoder's
 * (src/rle8_extreme_cpu.h:86-344, :936-1099, src/rleX_extreme_cpu_encode.h, src/rleX_Xsl.h, src/rleX_Xsl_short.h), written by many
 * lanes -- the input is cut behind runs that every encoder state stores, and the pieces are encoded by the block kernels
 * (csrc/hsrle_mono_encode.hip.h).  The codecs with a move-to-front list get the list in front of every piece from a dry pass, and the
 * result is checked piece by piece (wrong guesses are encoded again); HSRLE_ERR_UNSUPPORTED if that does not settle, and for the other
 * codecs (the drop-in functions then use one lane).
 * Round 6: rle8_multi / rle8_packed_multi do not use the block kernels' chunk mode any more -- a wave per chunk, then a wave per 4 KiB window
 * (csrc/hsrle_encode8pw.hip.h), nothing read back before the end.
 * dOut capacity >= rle_compress_bounds(inSize); dWorkspace >= hsrle_compress_mono_workspace_size(); synchronises `stream`.
 * hsrle_mono_encode_stats: of the calling thread's last list-codec encode: extra rounds, pieces encoded again in rounds 1 and 2,
 * pieces the final check rejected (0 unless the library is wrong).
 */
uint64_t hsrle_compress_mono_workspace_size(int codec, uint32_t inSize);
int hsrle_compress_mono_dev(int codec, const void *dIn, uint32_t inSize, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize, uint32_t *pStreamSize,
                            uint32_t *pChunks, void *stream);
void hsrle_mono_encode_stats(uint32_t stats[4]);
/*
 * rle8_multi / rle8_packed_multi (round 6: their chunks go to the windowed position-parallel encoder, csrc/hsrle_encode8pw.hip.h -- no chunk count, no step bound
 * and no list verdict has to come back to the host): the same encode without the host in the loop.  Nothing here synchronises or reads device memory, a HIP
 * graph can capture the call.  The stream's size is in its own header (bytes 4 .. 7, as the reference writes it: src/rle8_extreme_cpu.h:330-338) and, if
 * dStreamSize (DEVICE, 4 bytes) is not NULL, there.  HSRLE_ERR_UNSUPPORTED for every other codec: hsrle_compress_mono_dev_enqueue (below) takes the plain,
 * Packed and Short codecs of wider symbols, with a device status word; hsrle_compress_mono_dev the rest.
 */
int hsrle_compress_mono_dev_async(int codec, const void *dIn, uint32_t inSize, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize, uint32_t *dStreamSize,
                                  void *stream);
/*
 * The enqueue-only encode of ONE monolithic reference stream for every codec whose encoder state at a cut is fixed by the cut itself: rle8_multi,
 * rle8_packed_multi, the plain and Packed codecs of 16 .. 64 bit symbols (rle{16,24,32,48,64}_{sym,sym_packed,byte,byte_packed}), the Short codecs with no list or
 * a one-symbol list (rle{16,24,32,48,64}_{sym,1symlut_sym,byte,1symlut_byte}_short, rle8_multi_short, rle8_1symlut_short) -- 44 codecs.  Their chunks go to the
 * windowed position-parallel encoders in their chunk mode (csrc/hsrle_encode8pw.hip.h, csrc/hsrle_encodeSpw.hip.h).  Nothing here synchronises or reads device
 * memory: a HIP graph can capture the call.  Every check happens on the host before anything is enqueued: HSRLE_ERR_UNSUPPORTED for the other codecs (use
 * hsrle_compress_mono_dev), HSRLE_ERR_ARGUMENT / _CAPACITY / _DEVICE as for hsrle_compress_mono_dev.
 * dStatus (DEVICE, 4 bytes, required) receives HSRLE_MONO_DONE (dOut holds the stream; its size is in its bytes 4 .. 7) or HSRLE_MONO_ENCODE_FAILED (the
 * encode's own checks failed: dOut holds no stream).  dStreamSize (DEVICE, 4 bytes, may be NULL) receives the stream's size, 0 on failure.
 * dOut capacity >= rle_compress_bounds(inSize); dWorkspace >= hsrle_compress_mono_workspace_size().
 */
#define HSRLE_MONO_ENCODE_FAILED 4
int hsrle_compress_mono_dev_enqueue(int codec, const void *dIn, uint32_t inSize, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize,
                                    uint32_t *dStreamSize, uint32_t *dStatus, void *stream);
int hsrle_decompress_mono_dev(int codec, const void *dStream, uint32_t streamSize, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize,
                              uint32_t *pUncompressedSize, uint32_t *pStats, void *stream);
/*
 * The same without the host in the loop (nothing here synchronises or reads device memory: a HIP graph can capture the call).  The walk,
 * the proof, the entry records and the decode are enqueued in one go; the records pass is gated ON THE DEVICE by the proof's verdict.
 * pHeader16: the stream's first 16 bytes in HOST memory (zeros behind a stream shorter than that; the smallest stream is the codec's header, as for the
 * synchronous entry) (the caller read or received the stream; the launch geometry comes from the two
 * sizes and the mode byte in it -- rle8_extreme_cpu.h:702-764).  dStatus (device, 4 bytes) receives HSRLE_MONO_DONE (dOut holds the
 * output), HSRLE_MONO_MALFORMED, or HSRLE_MONO_NEEDS_REPAIR: an entry guess of the walk did not hold on this stream -- dOut is
 * unspecified, call hsrle_decompress_mono_dev (which repairs; codecs whose junk walks do not die on random literals -- the non-Packed,
 * non-7-bit-range formats -- see this more often because the synchronous function's pilot pass is skipped here).
 */
#define HSRLE_MONO_DONE 0
#define HSRLE_MONO_MALFORMED 1
#define HSRLE_MONO_NEEDS_REPAIR 2
int hsrle_decompress_mono_dev_async(int codec, const void *dStream, const uint8_t *pHeader16, uint32_t streamSize, void *dOut, uint64_t outCapacity, void *dWorkspace,
                                    uint64_t workspaceSize, uint32_t *pUncompressedSize, uint32_t *dStatus, void *stream);
/* tuning / test knob of the monolithic decode: output bytes per decode lane (multiple of 128), stream bytes per index lane, look-back
 * bytes of the entry guess; 0 = the library's choice.  Any values give the same output: the index is proven, not assumed.
 * PROCESS-GLOBAL and meant for tests: the one exception to "no library-owned state" -- a thread that changes it between another thread's
 * hsrle_*_mono_workspace_size() and its hsrle_*_mono_dev() can leave that call with too small a workspace (it then returns
 * HSRLE_ERR_CAPACITY, it never writes out of bounds). */
void hsrle_mono_tuning(uint32_t blockSize, uint32_t regionSize, uint32_t lookBack);

/*
 * Seekable monolithic streams: a persistent entry-point index beside the stream (a SIDECAR: the stream itself stays byte-identical to the
 * reference's), and a decode of any byte range from it.
 *
 * The index of ONE monolithic stream is a 64-byte header and one entry record per `spacing` output bytes: the decoder state at that
 * position, as the monolithic decode proves it (csrc/hsrle_capi.hip documents the layout).  Little endian, no pointers: the bytes copied
 * to the host are a file that can be stored beside the stream and loaded again, into any buffer, for the stream at any 128-byte aligned
 * address.  The same stream and spacing always give the same index bytes (whatever the tuning knobs, repair rounds or addresses).
 * Records are 96 bytes: at spacing 256 the index is 37 % of the uncompressed size, at 4 KiB 2.3 %, at 64 KiB 0.15 %.
 *   spacing: 0 = the library's choice (the monolithic decode's own lane size), else a multiple of 128 in [128, 1 MiB].
 *   Every codec hsrle_decompress_mono_dev decodes, the 8 bit Single mode included (the records carry the Single flag and symbol).
 */
typedef struct hsrle_mono_index_info
{
  uint32_t version, codec;
  uint32_t uncompressedSize, compressedSize;   /* as in the stream's header */
  uint32_t spacing, recordCount, recordBytes;  /* recordCount = ceil(uncompressedSize / spacing), recordBytes = 96 */
  uint8_t streamHead[16];                      /* the stream's first min(16, compressedSize) bytes, zeros behind */
  uint64_t indexBytes;                         /* 64 + recordCount * recordBytes */
} hsrle_mono_index_info_t;

/* bytes of the index / of the build's device workspace; 0 for invalid arguments */
uint64_t hsrle_mono_index_size(int codec, uint32_t uncompressedSize, uint32_t compressedSize, uint32_t spacing);
uint64_t hsrle_mono_index_workspace_size(int codec, uint32_t uncompressedSize, uint32_t compressedSize, uint32_t spacing);
/* Build the index of the stream at dStream (128-byte aligned, readable up to streamSize + 64) into dIndex (16-byte aligned, indexCapacity >=
 * hsrle_mono_index_size()).  The walk, proof and repair rounds of hsrle_decompress_mono_dev without its decode.  SYNCHRONOUS: reads the stream
 * header and the proof's verdict back, may repair.  pInfo (optional) receives the header.  HSRLE_ERR_FORMAT for a malformed stream,
 * HSRLE_ERR_CAPACITY for a small index or workspace, HSRLE_ERR_ARGUMENT for a bad pointer, alignment or spacing. */
int hsrle_mono_index_build_dev(int codec, const void *dStream, uint32_t streamSize, uint32_t spacing, void *dIndex, uint64_t indexCapacity, void *dWorkspace,
                               uint64_t workspaceSize, hsrle_mono_index_info_t *pInfo, void *stream);
/* Validate an index header in host memory (magic, version, codec, record count against the sizes and spacing, size): HSRLE_ERR_FORMAT if bad. */
int hsrle_mono_index_info_host(const void *pIndex, uint64_t size, hsrle_mono_index_info_t *pInfo);
/*
 * Decode output bytes [offset, offset + length) of the stream into dOut[0, length) (any byte address; nothing outside it is written).  Only the
 * decode lanes offset / spacing .. (offset + length - 1) / spacing run, each from its record.  ENQUEUE-ONLY: nothing here synchronises or reads
 * device memory, a HIP graph can capture the call; the index was proven when it was built, so there is no NEEDS_REPAIR.
 * dStream as for hsrle_decompress_mono_dev; dIndex (device, 16-byte aligned) the index, `info` its header (host).  length == 0: HSRLE_OK, nothing
 * enqueued; offset + length > uncompressedSize or outCapacity < length: HSRLE_ERR_ARGUMENT, nothing enqueued.
 * dStatus (device, 4 bytes) receives HSRLE_MONO_DONE, HSRLE_MONO_MALFORMED (decoder error bits) or HSRLE_MONO_INDEX_MISMATCH: the stream's first
 * 16 bytes differ from the index's stream head (nothing is written then), or a record's tag of the stream bytes at its entry position does not
 * match (a stale index whose header happens to be equal).  After MISMATCH or MALFORMED the contents of dOut[0, length) are unspecified.
 */
#define HSRLE_MONO_INDEX_MISMATCH 3
int hsrle_mono_decompress_range_dev_async(const void *dStream, const void *dIndex, const hsrle_mono_index_info_t *info, uint64_t offset, uint64_t length,
                                          void *dOut, uint64_t outCapacity, uint32_t *dStatus, void *stream);

/* ---------------------------------------------------------------------------------------------------------- */
/* 2. device-resident block container API                                                                      */

/*
 * Container layout (little endian):
 *   [ 0] char     magic[8]  = "HSRLEKIT"
 *   [ 8] uint32_t version   = 1
 *   [12] uint32_t codec     (hsrle_codec_t)
 *   [16] uint64_t uncompressedSize
 *   [24] uint32_t blockSize (uncompressed bytes per block; the last block may be shorter)
 *   [28] uint32_t blockCount
 *   [32] uint64_t payloadSize (sum of the block streams)
 *   [40] uint64_t totalSize   (header + table + payload + 32 bytes of zero padding)
 *   [48] uint8_t  reserved[16]
 *   [64] uint64_t offset[blockCount + 1]   (relative to the payload start; offset[blockCount] == payloadSize)
 *   [64 + 8 * (blockCount + 1)] payload: block streams back to back, each a complete reference stream
 *       (any stream the reference's decoder of the codec accepts -- whatever encoder wrote it -- with ONE exception: a packet that produces no byte, i.e. no literal
 *       and a run of zero bytes, which only the sym-aligned Packed codecs of 3 .. 16 byte symbols and the sym-aligned list codecs of wider symbols can express and no
 *       encoder of the kit writes.  Every decoder here -- block, split, windowed, monolithic, drop-in -- refuses such a stream as malformed and writes nothing
 *       outside its output)
 *   32 zero bytes (lets the decoder use 16-byte vector loads up to the last stream byte)
 */
#define HSRLE_CONTAINER_HEADER_SIZE 64u
#define HSRLE_CONTAINER_TAIL_PAD 32u
#define HSRLE_DEFAULT_BLOCK_SIZE 4096u
#define HSRLE_MIN_BLOCK_SIZE 128u
#define HSRLE_MAX_BLOCK_SIZE (1u << 30)

typedef struct hsrle_container_info
{
  uint32_t version, codec;
  uint64_t uncompressedSize;
  uint32_t blockSize, blockCount;
  uint64_t payloadSize, totalSize;
} hsrle_container_info_t;

/* A block size for `inSize` input bytes that fills the GPU: the default (4096) when that gives at least 65536 blocks, else 2048
 * or 1024.  One lane walks one block, so a buffer with few blocks is bound by the per-block latency (32 steps of ~8 us for 4 KiB),
 * not by bandwidth: an 88 MB frame decodes at 250 GiB/s with 4 KiB blocks and at 770 GiB/s with 1 KiB blocks -- for 9 % more
 * compressed bytes (every block carries its own stream header and terminator).  The choice is the caller's; nothing in the
 * library calls this on its own. */
uint32_t hsrle_suggest_block_size(uint64_t inSize);

/* Upper bound of the container size for `inSize` input bytes cut into blocks of `blockSize` (0 = default). */
uint64_t hsrle_container_bound(uint64_t inSize, uint32_t blockSize);
/* Scratch the compressor needs in device memory (per-block staging streams, sizes, scan partials). */
uint64_t hsrle_compress_workspace_size(uint64_t inSize, uint32_t blockSize);
/* The same for ONE codec.  Equal to the above except for the 8-bit Single codecs (rle8_single_short too), the 128-bit codecs and the Greedy encoders with a one-symbol
 * list (rle{16..64}_1symlut_byte_short_compress_greedy) on containers of fewer than 131 072 blocks of 1 .. 4 KiB: they have no run list encoder, and their small containers are encoded chunk by chunk (cuts behind long runs inside the blocks)
 * only if the workspace holds the chunk tables and staging area (about 2.3 x the input); with the general size they take one lane per block. */
uint64_t hsrle_compress_workspace_size_codec(int codec, uint64_t inSize, uint32_t blockSize);

/*
 * Enqueue compression of dIn[0, inSize) (device memory) into the container at dOut (device memory, capacity
 * outCapacity >= hsrle_container_bound()).  dWorkspace may be NULL: the library then keeps a cached allocation of
 * its own (not graph-capturable).  `stream` is a hipStream_t (NULL = default stream).  Asynchronous: the
 * container (including its header with totalSize) is complete when the stream reaches this point.
 */
int hsrle_compress_dev_async(int codec, const void *dIn, uint64_t inSize, void *dOut, uint64_t outCapacity,
                             uint32_t blockSize, void *dWorkspace, uint64_t workspaceSize, void *stream);
/* Same, then waits for the stream and returns the container size. */
int hsrle_compress_dev(int codec, const void *dIn, uint64_t inSize, void *dOut, uint64_t outCapacity,
                       uint32_t blockSize, uint64_t *pContainerSize, void *stream);

/* Read (device -> host, synchronising `stream`) and validate a container header. */
int hsrle_container_info_dev(const void *dContainer, uint64_t containerSize, hsrle_container_info_t *pInfo, void *stream);
/* Validate a container header that is already in host memory. */
int hsrle_container_info_host(const void *pContainer, uint64_t containerSize, hsrle_container_info_t *pInfo);

/*
 * Enqueue decompression of a container in device memory into dOut (device memory, capacity >= uncompressedSize;
 * no slack is needed and nothing outside [0, uncompressedSize) is written).  `info` must describe the container
 * (from hsrle_container_info_dev, or remembered from compression).  dStatus (device uint32_t, may be NULL) receives 0 or
 * a non-zero error mask if a block stream is malformed.
 */
int hsrle_decompress_dev_async(const void *dContainer, const hsrle_container_info_t *info, void *dOut, uint64_t outCapacity,
                               uint32_t *dStatus, void *stream);
/* Same, including the header read, a wait on the stream and the status check. */
int hsrle_decompress_dev(const void *dContainer, uint64_t containerSize, void *dOut, uint64_t outCapacity,
                         uint64_t *pUncompressedSize, void *stream);

/* Decode only blocks [firstBlock, firstBlock + blockCount) of a container into dOut + firstBlock * blockSize
 * (used by the multi-GPU sharding: every rank decodes its contiguous block range). */
int hsrle_decompress_blocks_dev_async(const void *dContainer, const hsrle_container_info_t *info, uint32_t firstBlock, uint32_t blockCount,
                                      void *dOut, uint64_t outCapacity, uint32_t *dStatus, void *stream);

/*
 * Decode output bytes [offset, offset + length) of a container into dOut[0, length) (any byte address; nothing outside it is written): one lane
 * per covering block, started from the block's header.  No parallelism inside a block: a range in one huge block is decoded from that
 * block's start by one lane.  ENQUEUE-ONLY (graph-capturable).  length == 0: HSRLE_OK, nothing enqueued; offset + length > uncompressedSize or
 * outCapacity < length: HSRLE_ERR_ARGUMENT, nothing enqueued.  dStatus (device, 4 bytes, required) receives HSRLE_MONO_DONE or HSRLE_MONO_MALFORMED.
 */
int hsrle_decompress_range_dev_async(const void *dContainer, const hsrle_container_info_t *info, uint64_t offset, uint64_t length, void *dOut,
                                     uint64_t outCapacity, uint32_t *dStatus, void *stream);

/*
 * Split decode: for containers with too few blocks to fill the GPU with one lane per block (one lane walks one block's packet chain:
 * ~10^5 blocks are needed; BASELINE config 3, an 88 MB frame in 4 KiB blocks, has 21 600).  One lane per block first walks the block's
 * packets and leaves the decoder state at every subBlockSize output bytes (csrc/hsrle_index.hip.h), then the block kernel runs one lane
 * per SUB-block.  The container, its block size and its compression ratio are what they are: nothing is re-encoded.
 * Round 4 -- the packet list decode (subBlockSize = HSRLE_SPLIT_PACKET_LIST, the library's choice for blocks of 256 bytes .. 16 KiB): the
 * walk leaves one 64-bit entry per PACKET (where its output starts, its literals, its symbol) instead of decoder states, and a second kernel
 * builds the output with one lane per 16 output bytes -- the packet chain is walked once, nothing else is sequential.
 *   subBlockSize: HSRLE_SPLIT_PACKET_LIST, or a multiple of 128 that divides blockSize (records at every subBlockSize bytes); 0 = the
 *   library's choice (hsrle_split_sub_block_size tells which; when it returns blockSize no split happens and no workspace is needed).
 *   dWorkspace (16-byte aligned) >= hsrle_decompress_split_workspace_size(info, blockCount, subBlockSize) bytes -- for the packet list
 *   about the uncompressed size of the blocks (blockSize / 8 + 2 entries per block: a block with more packets than that is finished by
 *   the walking lane, byte by byte).  Only enqueues kernels: graph-capturable.  dStatus as in hsrle_decompress_dev_async.
 */
#define HSRLE_SPLIT_PACKET_LIST 1u
uint32_t hsrle_split_sub_block_size(const hsrle_container_info_t *info, uint32_t subBlockSize);
uint64_t hsrle_decompress_split_workspace_size(const hsrle_container_info_t *info, uint32_t blockCount, uint32_t subBlockSize);
int hsrle_decompress_split_dev_async(const void *dContainer, const hsrle_container_info_t *info, uint32_t firstBlock, uint32_t blockCount, void *dOut, uint64_t outCapacity,
                                     uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize, uint32_t subBlockSize, void *stream);

#ifdef HSRLE_EXPERIMENTS
/*
 * EXPERIMENT BUILDS ONLY (-DHSRLE_EXPERIMENTS; the shipped library does not export this symbol).  Wave decode: one WAVE per block
 * (csrc/experiments/hsrle_decode_wave.hip.h) -- the block's stream goes to LDS, one lane hops through its packets leaving a descriptor
 * each, all 64 lanes expand them to whole aligned 16-byte stores.  Block sizes up to 16 KiB.  Measured slower than the split decode on the
 * 88 MB frame (427 against 189 us), which is why it does not ship.
 */
int hsrle_decompress_wave_dev_async(const void *dContainer, const hsrle_container_info_t *info, uint32_t firstBlock, uint32_t blockCount, void *dOut, uint64_t outCapacity,
                                    uint32_t *dStatus, void *stream);
#endif

/*
 * 64 bit hash of every block stream of blocks [firstBlock, firstBlock + blockCount) of a device-resident container into dHashes
 * (device, blockCount values): an integrity check that covers EVERY block (the big-config manifests under tests/golden/big/ hold the
 * reference encoder's values).  For the bytes p[0, len) of a stream:
 *   h = 0x9E3779B97F4A7C15 ^ (len * 0xD6E8FEB86659FD93);
 *   for every 8-byte little-endian word w (the last one zero padded): h = rotl64(h ^ w, 27) * 0x9E3779B97F4A7C15 + 0x165667B19E3779F9;
 *   h ^= h >> 31
 */
int hsrle_hash_blocks_dev_async(const void *dContainer, const hsrle_container_info_t *info, uint32_t firstBlock, uint32_t blockCount, uint64_t *dHashes, void *stream);

/* ---------------------------------------------------------------------------------------------------------- */
/* 3. host convenience wrappers (allocate device buffers, copy, run 2, copy back)                              */

int hsrle_compress_host(int codec, const void *pIn, uint64_t inSize, void *pOut, uint64_t outCapacity, uint32_t blockSize, uint64_t *pContainerSize);
int hsrle_decompress_host(const void *pContainer, uint64_t containerSize, void *pOut, uint64_t outCapacity, uint64_t *pUncompressedSize);

/* ---------------------------------------------------------------------------------------------------------- */
/* 4. multi-GPU: the path shards by independent blocks -- rank r of W encodes / decodes the contiguous block range
 *    [r * n / W, (r + 1) * n / W) with sections 2 of this header and needs no collective for that.  The ONE exchange step is
 *    assembling one container from the per-rank containers (and cutting one into per-rank containers); these functions do it over
 *    RCCL (xGMI inside a node): an all-gather of the per-rank sizes, then grouped point-to-point transfers of [offset table | payload]
 *    straight into their final places, offsets re-based by a small kernel.  One process per GPU; the communicator belongs to the caller.
 *    RCCL is loaded on first use (librccl.so.1); HSRLE_ERR_UNSUPPORTED if it is not there.  The reference has nothing comparable (it
 *    is single device); its closest precedent is the sub-section container of rle8m (src/rle8_low_entropy_cpu.c:131-191).             */

#define HSRLE_RCCL_ID_BYTES 128
/* rank 0: a fresh id (ncclGetUniqueId) to be handed to every rank by whatever the host program uses (MPI, torch.distributed, a file) */
int hsrle_rccl_unique_id(void *id128);
/* every rank, on its current HIP device: ncclCommInitRank.  *pComm is an ncclComm_t; a communicator the program already has works too */
int hsrle_rccl_comm_create(const void *id128, int worldSize, int rank, void **pComm);
int hsrle_rccl_comm_destroy(void *comm);
/* what the communicator itself says it spans (ncclCommCount / ncclCommUserRank): the figure a benchmark line should carry, not WORLD_SIZE */
int hsrle_rccl_comm_ranks(void *comm, int *pWorldSize, int *pRank);
/*
 * Collective over `comm`.  dLocal / localSize: this rank's container (device memory; NULL / 0 if the rank owns no block).  On the root,
 * dOut (device, capacity >= the sum of the parts, at most hsrle_container_bound(totalUncompressedSize, blockSize)) receives the one
 * container; *pTotalSize its size (every rank learns it).  All non-empty ranks must agree on codec and block size (HSRLE_ERR_FORMAT).
 * Enqueues on `stream` after two small synchronising reads (header, sizes).
 */
int hsrle_gather_container_rccl(void *comm, int root, const void *dLocal, uint64_t localSize, uint64_t totalUncompressedSize, void *dOut, uint64_t outCapacity,
                                uint64_t *pTotalSize, void *stream);
/* The inverse: the root's container is cut into one container per rank (contiguous block ranges, blocks renumbered from 0). */
int hsrle_scatter_container_rccl(void *comm, int root, const void *dContainer, uint64_t containerSize, void *dLocal, uint64_t localCapacity, uint64_t *pLocalSize, void *stream);

/* ---------------------------------------------------------------------------------------------------------- */
/* synthetic workloads of BASELINE.json generated directly in device memory (bench / tests)     */

#define HSRLE_SYNTH_RUNS 0  /* run-distributed(W): ~50 % of the bytes in runs, mean segment ~32 symbols          */
#define HSRLE_SYNTH_VIDEO 1 /* video-frame-shaped: zero dominated, short bursts of small values                  */
int hsrle_synth_dev_async(int kind, int symbolBytes, uint64_t seed, void *dOut, uint64_t size, void *stream);

/* library / device introspection */
int hsrle_device_count(void);

/* 1 if the library was built with -DHSRLE_EXPERIMENTS (developer builds: environment knobs that force kernel variants, kernels that were
 * measured slower than the shipped ones), 0 for the shipped build: no environment variable is read in any launch path. */
/* Memory the library keeps: calls that are given no workspace (hsrle_compress_dev, hsrle_decompress_dev, the host-pointer functions)
 * take their scratch stream-ordered from a memory pool the LIBRARY owns on the calling thread's device -- never from the device's default
 * pool, whose settings belong to the application.  Freed scratch stays in that pool up to the retention (default 2 GiB; UINT64_MAX keeps
 * everything, 0 returns everything at the next synchronisation); hsrle_trim() returns what the pool holds to the driver now.  Calls that
 * are handed their workspace (the *_async forms) allocate nothing.
 * hsrle_scratch_retention(bytes) applies the value to the pool of the calling thread's CURRENT device and makes it the default of every
 * pool the library creates later (one per device, on first use); pools that already exist on other devices keep their setting until the
 * function is called with that device current.  hsrle_trim() likewise acts on the current device's pool only. */
int hsrle_scratch_retention(uint64_t bytes);
int hsrle_trim(void);

int hsrle_experiments_enabled(void);

/* Which encoder hsrle_compress_dev[_async] uses for a container of `uncompressedSize` bytes in blocks of `blockSize` (no device needed;
 * the streams are the reference's whichever it is -- this is for capacity planning and for reading profiles):
 *   HSRLE_PATH_RING      one lane per block (the ring encoders): containers of >= 131 072 blocks, and whatever the other two do not take
 *   HSRLE_PATH_SPLIT     small containers, chunks inside the blocks
 *   HSRLE_PATH_RUN_LIST  small containers of 1 .. 4 KiB blocks, a wave per block
 * -1: bad codec / block size / size. */
#define HSRLE_PATH_RING 0
#define HSRLE_PATH_SPLIT 1
#define HSRLE_PATH_RUN_LIST 2
#define HSRLE_PATH_POSITION_PARALLEL 3   /* round 5: one wave per block, blocks of at most 4 KiB, any number of them: rle8_multi, rle8_packed_multi, the plain / Packed codecs of 2 .. 8 byte symbols, the 3 symbol LUT codecs of 3 .. 8 byte symbols, the Short codecs with no / one symbol in the list (1 .. 8 byte symbols) and with three (6 / 8 byte symbols): 56 codecs */
/* round 6: ... and, with blocks ABOVE 4 KiB walked in 4 KiB windows (a wave per block, then a wave per window: csrc/hsrle_encode8pw.hip.h, hsrle_encodeSpw.hip.h,
 * hsrle_encodeLpw.hip.h): rle8_multi / rle8_packed_multi and the plain / Packed codecs of 2 .. 8 byte symbols with blocks of any size; every LUT codec and the
 * position-parallel Short codecs with blocks below 1 MiB: 86 codecs (not: the 8 bit Single codecs, the 128 bit codecs) */
/* The answer is that of a workspace sized by hsrle_compress_workspace_size (no split regions for blocks of 1 .. 4 KiB): the library's own scratch and a workspace of
 * hsrle_compress_workspace_size_codec send the small containers of the Greedy codecs with a one-symbol list to HSRLE_PATH_SPLIT where this says HSRLE_PATH_RING. */
int hsrle_encode_path(int codec, uint64_t uncompressedSize, uint32_t blockSize);

/* Which stream ring (bytes per lane in LDS: 64 or 128) the block decoder of hsrle_decompress_dev_async / hsrle_decompress_blocks_dev_async takes for a
 * container of this codec with these header fields (no device needed; the output is the same bytes whichever it is -- this is for reading profiles and
 * for tests that must know which kernel they ran).  Containers whose streams shrink far enough take the instantiation with the small ring: 1 .. 4 byte
 * symbols only, the threshold goes by the symbol width (csrc/hsrle_codecs.h: small_ring_per_mille).  A block range of a container takes what the whole
 * container takes.  Launches from entry records (split decode by sub-blocks, monolithic streams) and with an output window
 * (hsrle_decompress_range_dev_async) always use 128 and are not what this reports; nor is hsrle_decompress_dev, which takes the split decode (no ring, or 128) for
 * every container of fewer than 131 072 blocks and this kernel only above.  -1: bad codec. */
int hsrle_decode_ring(int codec, uint64_t uncompressedSize, uint64_t payloadSize);

/* A hash of the library's sources and build flags (set by the Makefile; "unknown" for other build recipes): measurement files that
 * describe one build of the kernels (profiles/r03_traffic.json) carry it, and bench.py refuses a file of another build. */
const char *hsrle_build_id(void);
/* Workgroups (= wavefronts: every kernel here runs one wave per workgroup) of the codec's decode (decode != 0) or encode kernel
 * that are resident on one CU at a time, as the HIP runtime computes it from the kernel's LDS and register use; 0 on error.
 * The kernels are latency bound, so this is the first number to look at when a build got slower. */
/* ---------------------------------------------------------------------------------------------------------- */
/* rle8m: the reference's own GPU decode path.  `rle8m_opencl_*` are the names of      */
/* src/rle.h:464-466 (src/rle8_ocl.c:56, :185, :265); `rle8m_decompress` is the CPU twin of the same format   */
/* (src/rle.h:63, src/rle8_low_entropy_cpu.c:193-250).  Host pointers; one wave (few or large sub-sections)  */
/* or one lane (many small ones) decodes one sub-section.                                                     */
bool rle8m_opencl_init(const size_t inputDataSize, const size_t outputDataSize, const size_t maxSubsectionCount);
void rle8m_opencl_destroy(void);
uint32_t rle8m_opencl_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8m_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);

/* rle8m encode, the GPU twin of the reference's CPU function (src/rle.h:61-62, src/rle8_low_entropy_cpu.c:126-191): same stream,
 * same failure rule (0 when a section outgrows what is left of the output at its turn) -- plus one the reference lacks: 0 as well
 * when a section's STREAM (up to twice the section) does not fit, where the reference writes behind pOut + outSize.           */
uint32_t rle8m_compress_bounds(const uint32_t subSections, const uint32_t inSize);
uint32_t rle8m_compress(const uint32_t subSections, const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
/* device-resident encode: only enqueues kernels; *dStatus != 0 afterwards = the reference would have returned 0 */
/* The UNSECTIONED forms of the same codec (src/rle.h:53-57, :90-93; src/rle8_low_entropy_cpu.c:6-124,
 * src/rle8_low_entropy_short_cpu.c:16-124): [u32 compressedSize][u32 uncompressedSize][info][ONE stream], i.e. an rle8m stream of one
 * section without its section-count field.  Same names, arguments and return convention as the reference (0 = failure); the streams are
 * the reference's byte for byte, the decoders read the reference's streams.  The Short form cuts runs every 32 bytes instead of 255;
 * *_only_max_frequency lets one symbol -- the one that saves the most -- carry repeat codes.  The one stream is worked on by many waves:
 * the encoder cuts its input at run boundaries (no token crosses one), the decoder cuts the stream anywhere and finds out from the byte
 * values in front of a cut whether it starts with a symbol or a repeat code (csrc/hsrle_rle8m.hip.h).  Unlike the reference a stream that
 * outgrows `outSize` is a failure, never a write behind the caller's buffer (rle8_low_entropy_cpu.c:476 only asks for outSize >= inSize).
 * The split-phase helpers that pass the codec's tables through host structs follow below. */
uint32_t rle8_low_entropy_compress_bounds(const uint32_t inSize);
uint32_t rle8_low_entropy_decompressed_size(const uint8_t *pIn, const uint32_t inSize);
uint32_t rle8_low_entropy_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_low_entropy_compress_only_max_frequency(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_low_entropy_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_low_entropy_short_compress_bounds(const uint32_t inSize);
uint32_t rle8_low_entropy_short_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_low_entropy_short_compress_only_max_frequency(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_low_entropy_short_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);

/* The split-phase helpers of the same codec (src/rle.h:67-96; src/rle8_low_entropy_cpu.c:254-600, :930-1022, src/rle8_low_entropy_short_cpu.c:128-534):
 * the statistics pass, the header writer / reader and the two stream bodies as separate calls, tables handed through host structs with the
 * reference's layout.  rle8_low_entropy_compress is exactly  [u32 size][u32 inSize] + write_compress_info(get_compress_info) +
 * compress_with_info,  as in the reference (rle8_low_entropy_cpu.c:11-50), and the tests check that identity.
 *   get_compress_info*      statistics + tables on the GPU (k_rle8m_stats_wave, k_rle8m_info), false = bad arguments / no device
 *   write_compress_info     host only: 32 flag bytes, the symbol count (a uint8: 256 symbols are written as 0 and then 255 of them, sic), the symbols
 *   compress_with_info      the stream body for ANY tables (rle[] / symbolsByProb[] need not come from get_compress_info); returns its size,
 *                           0 = failure.  Unlike the reference a body that outgrows `outSize` is a failure, not a write behind the buffer.
 *   read_decompress_info    host only; returns the bytes of the info (33 + listed symbols)
 *   decompress_with_info    pIn .. pEnd = the body; returns expectedOutSize, 0 = malformed body or tables that are not a permutation
 *                           (the reference returns expectedOutSize whatever it read)                                                  */
typedef struct rle8_low_entropy_compress_info_t { bool rle[256]; uint8_t symbolsByProb[256]; uint8_t symbolCount; } rle8_low_entropy_compress_info_t;   /* src/rle.h:67-72 */
typedef struct rle8_low_entropy_decompress_info_t { bool rle[256]; uint8_t symbolToCount[256]; } rle8_low_entropy_decompress_info_t;                     /* src/rle.h:81-85 */
bool rle8_low_entropy_get_compress_info(const uint8_t *pIn, const uint32_t inSize, rle8_low_entropy_compress_info_t *pCompressInfo);
bool rle8_low_entropy_get_compress_info_only_max_frequency(const uint8_t *pIn, const uint32_t inSize, rle8_low_entropy_compress_info_t *pCompressInfo);
uint32_t rle8_low_entropy_write_compress_info(rle8_low_entropy_compress_info_t *pCompressInfo, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_low_entropy_compress_with_info(const uint8_t *pIn, const uint32_t inSize, const rle8_low_entropy_compress_info_t *pCompressInfo, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_low_entropy_read_decompress_info(const uint8_t *pIn, const uint32_t inSize, rle8_low_entropy_decompress_info_t *pDecompressInfo);
uint32_t rle8_low_entropy_decompress_with_info(const uint8_t *pIn, const uint8_t *pEnd, const rle8_low_entropy_decompress_info_t *pDecompressInfo, uint8_t *pOut, const uint32_t expectedOutSize);
uint32_t rle8_low_entropy_short_compress_with_info(const uint8_t *pIn, const uint32_t inSize, const rle8_low_entropy_compress_info_t *pCompressInfo, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_low_entropy_short_decompress_with_info(const uint8_t *pIn, const uint8_t *pEnd, const rle8_low_entropy_decompress_info_t *pDecompressInfo, uint8_t *pOut, const uint32_t expectedOutSize);

/* The same, device resident (variant: bit 0 the Short form, bit 1 only_max_frequency).  Compress only enqueues (the stream's size is its
 * first u32; *dStatus != 0: the stream did not fit `outCapacity`); decompress reads the header and the verdict (two stream synchronisations).
 * A stream that is refused (HSRLE_ERR_FORMAT) leaves nothing written outside dOut[0 .. outCapacity); what dOut itself holds then is not defined.
 *   For tests and measurements: behind a decompress call that got as far as decoding, word 2 of the workspace (bytes 8 .. 11) is the number of
 *   decode attempts: 1 = many waves on the one stream; 2 = a piece of the stream had 65 536 or more flagged-valued bytes right in front of it, the
 *   backward scan for its symbol / code parity gave up, and ONE wave decoded the whole stream once more (same bytes, much slower).
 * Every decoder of this codec here -- these, the drop-in names above and the rle8m ones -- reads the header as its grammar says: of two listings of
 * one symbol the last one counts (as in the reference, rle8_low_entropy_cpu.c:579-584), and a stream in which all 256 symbols carry repeat codes
 * decodes like any other.  The reference counts the flagged symbols in a uint8_t (rle8_low_entropy_cpu.c:940-945): 256 wrap to 0, it then copies
 * the stream as if nothing were flagged and does not give back what its own encoders wrote (2 304 bytes -- the 256 values in runs of 3, three times over --
 * are such an input).  That is not reproduced.
 * The two encoders (hsrle_low_entropy_compress_dev_async, hsrle_rle8m_compress_dev_async): dIn and dOut at any byte address; dWorkspace 16-byte aligned, its
 * contents do not matter; dStatus ONE device word, 4-byte aligned (or NULL) -- a misaligned workspace or status word is HSRLE_ERR_ARGUMENT.  HSRLE_ERR_ARGUMENT and
 * HSRLE_ERR_CAPACITY mean that nothing was enqueued and nothing written.  What a call leaves in dOut behind the stream's end is not defined.
 *   For tests and measurements: behind either compress call the first 2 048 bytes of the workspace are the run statistics the tables were made from --
 *   prob[256], then pcount[256], uint32 each (a maximal run of L bytes adds L to prob and L / 255 + 1 to pcount -- L / 32 + 1 for the Short form -- and the
 *   run that ends the input adds 1 to pcount whatever its length, rle8_low_entropy_cpu.c:264-296). */
uint64_t hsrle_low_entropy_workspace_size(uint32_t inSize);
int hsrle_low_entropy_compress_dev_async(const void *dIn, uint32_t inSize, int variant, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize, uint32_t *dStatus, void *stream);
uint64_t hsrle_low_entropy_decompress_workspace_size(uint64_t streamSize);
int hsrle_low_entropy_decompress_dev(const void *dStream, uint64_t streamSize, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize, uint32_t *pUncompressedSize, void *stream);

uint64_t hsrle_rle8m_compress_workspace_size(uint32_t inSize, uint32_t sections);
int hsrle_rle8m_compress_dev_async(const void *dIn, uint32_t inSize, uint32_t sections, void *dOut, uint64_t outCapacity, void *dWorkspace, uint64_t workspaceSize,
                                   uint32_t *dStatus, void *stream);

/* device-resident form: the stream header is read once (synchronises), the decode only enqueues a kernel */
typedef struct hsrle_rle8m_info { uint32_t compressedSize, uncompressedSize, sections; } hsrle_rle8m_info_t;
int hsrle_rle8m_info_dev(const void *dStream, uint64_t streamSize, hsrle_rle8m_info_t *pInfo, void *stream);
int hsrle_rle8m_decompress_dev_async(const void *dStream, const hsrle_rle8m_info_t *info, void *dOut, uint64_t outCapacity, uint32_t *dStatus, void *stream);

/* ---------------------------------------------------------------------------------------------------------- */
/* 5. the multi-move-to-front transforms (src/rle.h:420-438; src/mmtf.c, src/bit_mmtf.c): preconditioning steps that keep the size.     */
/* mmtf128 / mmtf256: 16 / 32 interleaved byte columns, each with its own move-to-front list; encode writes ranks, decode symbols; the    */
/* inSize % 16 (32) bytes behind the last whole row are looked up without an update.  bitmmtf8 / bitmmtf16: XOR with the previous byte /  */
/* little-endian 16 bit word (an odd last byte of bitmmtf16 is copied).  Same names, arguments and return values as the reference: inSize */
/* on success, 0 for inSize == 0, inSize > outSize, a NULL pointer or no usable device.  Host pointers, staged per device like section 1. */
/* rle8_mmtf128_* (RLE + MMTF + bit packing, rle.h:442-452) and rle8_sh_* (rle.h:455-458) follow below.  Still open of rle.h: only          */
/* rle8_mmtf256_compress / _decompress, which the reference declares and never defines.                                                    */
uint32_t mmtf_bounds(const uint32_t inSize);
uint32_t mmtf128_encode(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t mmtf128_decode(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t mmtf256_encode(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t mmtf256_decode(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t bitmmtf_bounds(const uint32_t inSize);
uint32_t bitmmtf8_encode(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t bitmmtf8_decode(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t bitmmtf16_encode(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t bitmmtf16_decode(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);

/*
 * The same, device resident and ENQUEUE-ONLY: nothing here allocates, synchronises or reads device memory, a HIP graph can capture the call, and it
 * composes with hsrle_compress_dev_async / hsrle_decompress_dev_async on one stream.  dIn / dOut at any byte address, not overlapping; exactly `size`
 * bytes are written.  dWorkspace >= hsrle_mmtf_workspace_size(transform, size) bytes at any address, its contents do not matter.  The move-to-front
 * transforms cut the rows into segments (a lane per segment and column; csrc/hsrle_mmtf.hip.h) and keep 256 bytes of state per segment and column in
 * the workspace: at most size / 8 + 1 MiB.  HSRLE_ERR_ARGUMENT: NULL pointer, unknown transform, size > 2^32 - 1, overlapping buffers;
 * HSRLE_ERR_CAPACITY: short workspace; size == 0: HSRLE_OK, nothing is launched.  hsrle_mmtf_workspace_size: 0 for an unknown transform or such a size.
 * hsrle_mmtf_tuning: rows per segment of mmtf128 / mmtf256 and elements per chunk of the bitmmtf decodes (the prefix XOR is a reduction per chunk, a
 * scan of the chunk values and an apply pass); 0 = the library's choice.  Any value gives the same bytes.  PROCESS-GLOBAL and meant for tests, like
 * hsrle_mono_tuning: it changes the workspace size.
 */
#define HSRLE_MMTF128 0
#define HSRLE_MMTF256 1
#define HSRLE_BITMMTF8 2
#define HSRLE_BITMMTF16 3
uint64_t hsrle_mmtf_workspace_size(int transform, uint64_t size);
int hsrle_mmtf_dev_async(int transform, int decode, const void *dIn, uint64_t size, void *dOut, void *dWorkspace, uint64_t workspaceSize, void *stream);
void hsrle_mmtf_tuning(uint32_t segmentRows);

/*
 * rle8_mmtf128 (src/rle8_mmtf.c, rle.h:442-452): the mmtf128 transform, run-length coding over the 16-byte rank rows, 2 / 3 / 4 bit packing of the
 * literal rows -- one stream: u32 inSize, u32 streamSize, COPY and RLE packets in turn, the inSize % 16 tail ranks (csrc/hsrle_rle8mmtf.hip.h has the
 * grammar).  Same names, arguments and return values as the reference.  bounds: 0 above 2^30, else inSize + 8.  compress: the stream's size; 0 for a
 * NULL pointer, inSize == 0, outSize < bounds.  decompress: the header's inSize; 0 for a NULL pointer, a zero size, header sizes larger than the
 * arguments.  rle8_mmtf256_compress / _decompress are only declared by the reference (no body anywhere) and are NOT exported; the bounds function is.
 * Where this library differs, on purpose:
 *  - THE FIRST PACKET'S WIDTH.  The reference ORs an undefined start value (_mm_undefined_si128, rle8_mmtf.c:182) into the width decision of the first
 *    COPY packet, so its first packet may be wider than its rows need, differently from build to build.  Here the start value is ZERO: the first
 *    packet gets the narrowest width its rows allow (a first COPY of no rows is the byte 0x06).  Whenever a row of the first packet holds a rank
 *    >= 16 the reference is deterministic too and the streams are equal byte for byte; otherwise they are equal from the end of the first COPY
 *    packet on, and each side decodes the other's stream.
 *  - compress returns 0 for inSize > 2^30 (the reference's bound is 0 there and it runs on).
 *  - The reference's bound forgets the 8 header bytes: incompressible input of 32 rows or more needs up to inSize + 13 and the reference writes
 *    past outSize.  compress returns 0 when the stream does not fit in outSize; inSize + 13 bytes always suffice.
 *  - decompress checks every packet against streamSize and the row count BEFORE anything is written and returns 0 for a malformed stream (a packet
 *    past the stream's end or the last row, a chain that has not ended when the rows are used up, rows left over, inSize < 8); the reference does
 *    not check.
 * Host pointers, staged per device like the functions above.
 */
uint32_t rle8_mmtf128_compress_bounds(const uint32_t inSize);
uint32_t rle8_mmtf256_compress_bounds(const uint32_t inSize);
uint32_t rle8_mmtf128_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_mmtf128_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);

/*
 * The same, device resident and ENQUEUE-ONLY (nothing allocates, synchronises or reads device memory; a HIP graph can capture the calls; nothing is
 * zeroed, every word the kernels read is written by a kernel before).  Buffers at any byte address, not overlapping; dOutSize / dStatus: device words,
 * 4-byte aligned.  dWorkspace >= hsrle_rle8_mmtf128_workspace_size(decode, uncompressed size) bytes, contents do not matter: the rank buffer (the
 * uncompressed size), 16 bytes per span of 64 rows twice (compress) or 16 bytes per row for the packet records (decompress), the mmtf128 workspace.
 * compress: 1 <= inSize <= 2^30 and outCapacity >= inSize + 8, else HSRLE_ERR_ARGUMENT / HSRLE_ERR_CAPACITY and nothing is enqueued.  *dOutSize
 *   receives the stream's size and *dStatus HSRLE_RLE8_MMTF_DONE, or 0 and HSRLE_RLE8_MMTF_CAPACITY when the stream is larger than outCapacity (see
 *   above; then nothing is written to dOut).
 * decompress: outSize is the UNCOMPRESSED size, which the caller knows (the stream's first word): the mmtf128 decode is planned from it on the host.
 *   The header is read on the device; *dStatus receives HSRLE_RLE8_MMTF_DONE, or HSRLE_RLE8_MMTF_MALFORMED (header inSize != outSize, header
 *   streamSize > streamSize, or a chain as described above); then dOut[0, outSize) holds nothing of use.  Never more than outSize bytes are written.
 *   The header chain is followed by ONE wave (the format's one serial dependence): its time grows with the number of packets, not the bytes.
 * hsrle_rle8_mmtf_tuning: rows per wave span of the compress passes, 1 .. 64 (0 or more = 64).  Any value gives the same bytes.  PROCESS-GLOBAL,
 * for tests; it changes the workspace size.  hsrle_mmtf_tuning acts on the mmtf128 passes inside as it does on their own.
 */
#define HSRLE_RLE8_MMTF_DONE 0
#define HSRLE_RLE8_MMTF_MALFORMED 1
#define HSRLE_RLE8_MMTF_CAPACITY 2
uint64_t hsrle_rle8_mmtf128_workspace_size(int decode, uint64_t size);
int hsrle_rle8_mmtf128_compress_dev_async(const void *dIn, uint64_t inSize, void *dOut, uint64_t outCapacity, uint32_t *dOutSize, uint32_t *dStatus, void *dWorkspace,
                                          uint64_t workspaceSize, void *stream);
int hsrle_rle8_mmtf128_decompress_dev_async(const void *dStream, uint64_t streamSize, void *dOut, uint64_t outSize, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize,
                                            void *stream);
void hsrle_rle8_mmtf_tuning(uint32_t spanRows);

/*
 * The ENTRY INDEX of one rle8_mmtf128 stream: a sidecar beside the stream (the stream does not change by a byte) that names packet headers of the chain,
 * so that the chain is followed by a wave per stretch between two entries instead of ONE wave.  Little endian, no pointers, position independent: the
 * bytes can be stored beside the stream and loaded into any buffer at any byte address.  The same stream and spacing always give the same index bytes,
 * whether the encoder wrote the index (compress_indexed) or the serial walk of a stream written elsewhere (index_build), whatever the tuning knobs.
 *   64 header bytes: "HSRLEMFI", u32 version = 1, u32 headerBytes = 64, u32 uncompressedSize, u32 streamSize (the stream header's second word),
 *     u32 spacingRows, u32 entryCount, u64 indexSize = 64 + 16 entryCount, zeros up to byte 64.
 *   entryCount entries of 16 bytes: u32 offset (from the start of the stream, of the packet's own header byte), u32 row (the packet's first 16-byte
 *     row), u32 ordinal (the non-null packets in front of it), u32 kind (0 COPY, 1 RLE).
 *   THE RULE (R = uncompressedSize / 16 rows): for every j >= 1 with j spacingRows < R the first non-null packet whose first row lies in
 *     [j spacingRows, (j + 1) spacingRows), if there is one, in order of j.  A window in which no packet begins has no entry; the chain's start (offset 8,
 *     row 0, ordinal 0, COPY) is not stored; of an RLE packet behind an RLE packet the entry is the RLE header, not the null COPY in front of it.
 *   spacingRows: a multiple of 64 in [64, 2^20]; 0 = 1024.  16 bytes per entry: at most 1 / spacingRows of the uncompressed size.
 * The info struct of these calls is hsrle_mono_index_info_t (section 1), as the block containers of this section share theirs: version = 1,
 * codec = HSRLE_RLE8_MMTF_INDEX_CODEC, compressedSize = streamSize, spacing = spacingRows, recordCount = entryCount, recordBytes = 16, streamHead = zeros,
 * indexBytes = indexSize.  hsrle_rle8_mmtf128_index_info_t is another name of it.
 *
 * THE INDEX IS TRUSTED IN NOTHING.  The indexed decode checks every entry (offset inside the stream, row below R, ordinal <= row, kind <= 1, offset, row
 * and ordinal strictly increasing) before it is used, and every stretch has to END STANDING ON the next entry's header in exactly that entry's row,
 * ordinal and kind; the first stretch starts at the chain's true start, so an index that passes has given the very record list of the plain decode.  An
 * index whose entries are true packet headers in order but not the rule's choice decodes correctly and is accepted: the decode proves entries, not
 * the rule.  Everything else is HSRLE_RLE8_MMTF_INDEX: a bad entry, a missed landing, any packet of a stretch that the plain decode would refuse, an index
 * header on the device that differs from `info`, a streamSize that is not the stream header's.  The verdict precedes every write outside the workspace;
 * after INDEX (and MALFORMED: the stream header against the arguments, as in the plain call) nothing outside dOut[0, outSize) is touched and dOut
 * holds nothing of use.  INDEX says that index and stream do not agree; whether the stream itself is malformed the plain call decides.
 *
 * hsrle_rle8_mmtf128_index_bound: an index capacity that always suffices; 0 for a bad spacing or a size above 2^30.
 * hsrle_rle8_mmtf128_index_info_host: validates a header in host memory (magic, version, spacing, entryCount against the sizes, indexSize against
 *   entryCount and `size`); HSRLE_ERR_FORMAT if bad.
 * The device calls are ENQUEUE-ONLY like the calls above (a HIP graph can capture them; buffers at any byte address; dOutSize / dStatus 4-byte aligned
 * device words, dIndexSize an 8-byte aligned device word).
 *   compress_indexed: hsrle_rle8_mmtf128_compress_dev_async (same arguments, same workspace, the same stream byte for byte) and the index from what its
 *     passes know: two small kernels behind it.  indexCapacity >= hsrle_rle8_mmtf128_index_bound(inSize, spacingRows), else HSRLE_ERR_CAPACITY.  On
 *     HSRLE_RLE8_MMTF_CAPACITY *dIndexSize is 0 and no header is written.
 *   index_build: the index of a stream written by anyone.  SERIAL BY NATURE: one wave follows the whole chain once, as the plain decode does on every
 *     call; it pays back on every later indexed decode.  No workspace.  *dStatus: DONE, or MALFORMED as the plain decode says it; then *dIndexSize is 0
 *     and the magic is not written.
 *   decompress_indexed: dIndex / info: the index and its header (host, from index_info_host or built from *dIndexSize and the rule's header fields);
 *     info->uncompressedSize == outSize, else HSRLE_ERR_ARGUMENT.  dWorkspace >= hsrle_rle8_mmtf128_workspace_size(1, outSize).  The grid is
 *     entryCount + 1 waves: a captured call replays on any stream and index of the same sizes and entry count.
 * The two host-pointer calls stage through the device like the functions above.  index_build_host: HSRLE_ERR_FORMAT for a malformed stream.
 * decompress_indexed_host: HSRLE_ERR_FORMAT for a bad index header and for a decode that did not end DONE.
 * Measured on an MI355X (profiles/r18_rle8_mmtf_index.md; 1 GiB device resident, spacing 1024, video-shaped / run-distributed / tiny packets): decompress
 * 3 368 / 3 611 / 18 201 ms plain, 7.4 / 30.2 / 12.3 ms indexed (the walk itself 1.3 / 1.3 / 6.7 ms); 256 and 4096 rows are within 2 % of 1024 at 1 GiB.
 * compress_indexed costs 5 ms over the plain compress at 1 GiB (15.9 -> 20.9, 92.5 -> 97.4, 13.0 -> 18.1 ms), 0.3 ms at 64 MiB; index_build costs one
 * plain decode's walk (3.5 / 3.7 / 19.2 s).  The index is 0.40 / 0.11 / 0.45 % of the stream.
 */
#define HSRLE_RLE8_MMTF_INDEX 3
#define HSRLE_RLE8_MMTF_INDEX_CODEC 0xFFFFFFFFu
typedef hsrle_mono_index_info_t hsrle_rle8_mmtf128_index_info_t;
uint64_t hsrle_rle8_mmtf128_index_bound(uint64_t uncompressedSize, uint32_t spacingRows);
int hsrle_rle8_mmtf128_index_info_host(const void *pIndex, uint64_t size, hsrle_mono_index_info_t *pInfo);
int hsrle_rle8_mmtf128_compress_indexed_dev_async(const void *dIn, uint64_t inSize, void *dOut, uint64_t outCapacity, uint32_t *dOutSize, uint32_t *dStatus, void *dWorkspace,
                                                  uint64_t workspaceSize, uint32_t spacingRows, void *dIndex, uint64_t indexCapacity, uint64_t *dIndexSize, void *stream);
int hsrle_rle8_mmtf128_index_build_dev_async(const void *dStream, uint64_t streamSize, uint64_t uncompressedSize, uint32_t spacingRows, void *dIndex, uint64_t indexCapacity,
                                             uint64_t *dIndexSize, uint32_t *dStatus, void *stream);
int hsrle_rle8_mmtf128_decompress_indexed_dev_async(const void *dStream, uint64_t streamSize, const void *dIndex, const hsrle_mono_index_info_t *info, void *dOut, uint64_t outSize,
                                                    uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize, void *stream);
int hsrle_rle8_mmtf128_index_build_host(const void *pStream, uint64_t streamSize, uint32_t spacingRows, void *pIndex, uint64_t indexCapacity, uint64_t *pIndexSize);
int hsrle_rle8_mmtf128_decompress_indexed_host(const void *pStream, uint64_t streamSize, const void *pIndex, uint64_t indexSize, void *pOut, uint64_t outCapacity,
                                               uint64_t *pUncompressedSize);

/*
 * BYTE-RANGE DECODE of one rle8_mmtf128 stream, and the CHECKPOINTS it needs: a second sidecar beside the stream and its entry index (neither changes by a
 * byte).  The index lets the header chain be entered in the middle; the sixteen move-to-front lists at a range's start depend on every byte in front of it,
 * and the checkpoints hold them.  Little endian, no pointers, position independent, at any byte address.
 *   64 header bytes: "HSRLEMFC", u32 version = 1, u32 headerBytes = 64, u32 uncompressedSize, u32 streamSize, u32 checkpointRows, u32 checkpointCount,
 *     u64 size = 64 + 4096 checkpointCount, zeros up to byte 64.
 *   checkpointCount checkpoints of 4096 bytes: checkpoint k = 1 .. count holds the sixteen lists of mmtf128 as they stand in front of row k checkpointRows,
 *     column c's at bytes [256 c, 256 c + 256), byte i the symbol of rank i.  With R = uncompressedSize / 16 rows, checkpointCount = (R - 1) / checkpointRows
 *     (0 for R = 0): row 0 is the identity and not stored, and there is none for the tail -- a range that touches the uncompressedSize % 16 tail bytes is
 *     decoded through row R.
 *   checkpointRows: a multiple of 64 in [64, 2^24]; 0 = 65 536 (1 MiB of output per checkpoint, 0.39 % of the uncompressed size).
 *   The lists are a function of the uncompressed bytes alone: the same data and checkpointRows give the same sidecar bytes, whatever the tuning knobs.
 * hsrle_rle8_mmtf128_checkpoints_info_t holds the header's fields.  The calls below take it through a void pointer (`checkpointsInfo`, `pInfo`): it always
 * points to this struct.
 *
 * NEITHER SIDECAR IS TRUSTED FOR MEMORY SAFETY.  Every entry and every packet is bounds-checked as in the indexed decode, the records a stretch may write are
 * bounded before it is walked, and a rank only ever indexes a 256-entry list: any bytes in either sidecar leave everything outside dOut[0, length) and the
 * workspace untouched.  But a range decode CANNOT PROVE CONTENT the way the whole indexed decode does: its first stretch starts from an entry that nothing
 * in front of it vouches for, and a checkpoint that is a permutation of 0 .. 255 but the wrong one gives wrong bytes with HSRLE_RLE8_MMTF_DONE.  The landing
 * rule still proves that consecutive entries inside the range agree with the stream.  The arbiter of both sidecars is decompress_indexed of the whole stream,
 * and checkpoints_build run again.  The record table is sized for an index by the rule (at most spacingRows packets between an entry and the range): a sparser
 * index of true headers, which decompress_indexed accepts, can end in HSRLE_RLE8_MMTF_INDEX here.
 *
 * hsrle_rle8_mmtf128_checkpoints_bound: the exact sidecar size; 0 for a bad checkpointRows or a size above 2^30.
 * hsrle_rle8_mmtf128_checkpoints_info_host: validates a header in host memory (magic, version, checkpointRows, the count against the sizes, `size`);
 *   HSRLE_ERR_FORMAT if bad.
 * The device calls are ENQUEUE-ONLY (a HIP graph can capture them; buffers at any byte address; dStatus a 4-byte aligned device word, dSize 8-byte aligned).
 *   checkpoints_build: from any stream and its index (indexInfo: its header, as for decompress_indexed).  One indexed decode without its last pass, and a
 *     lane per (checkpoint, column) behind it; a stream without an index pays index_build's serial walk first, once.  dWorkspace >=
 *     hsrle_rle8_mmtf128_workspace_size(1, uncompressedSize); capacity >= checkpoints_bound, else HSRLE_ERR_CAPACITY.  *dStatus: DONE, or MALFORMED / INDEX
 *     exactly as decompress_indexed says them; then *dSize is 0 and the magic is not written.
 *   decompress_range: output bytes [offset, offset + length) to dOut[0, length); nothing outside it and the workspace is written.  Only the stretches from the
 *     last entry at or in front of the checkpoint row c <= offset / 16 to the range's end are walked, only rows [c, end) expanded and transformed, from
 *     checkpoint c's lists (c = 0: the identity, no checkpoint is read).  length == 0: HSRLE_OK, nothing enqueued.  offset + length > uncompressedSize,
 *     outCapacity < length, two infos that disagree in uncompressedSize or streamSize: HSRLE_ERR_ARGUMENT, nothing enqueued.  dWorkspace >=
 *     hsrle_rle8_mmtf128_range_workspace_size(length, spacingRows, checkpointRows): a function of the range and the two spacings, never of the stream's size
 *     (0 for bad arguments).  *dStatus: DONE; MALFORMED (the stream header against the arguments); INDEX (the index header on the device differs from
 *     indexInfo, a bad entry, a missed landing, a packet the plain decode would refuse, a stretch with more packets than the record table holds); CHECKPOINT
 *     (the header on the device differs from checkpointsInfo, or a list of the checkpoint the range starts from is not a permutation of 0 .. 255).  Every
 *     verdict precedes every write to dOut: behind anything but DONE dOut is untouched.  A captured call replays on any stream, index and checkpoints of the
 *     same sizes and counts, for the same range.
 * The two host-pointer calls stage through the device like the functions above; HSRLE_ERR_FORMAT for a bad sidecar header and for a status that is not DONE.
 */
#define HSRLE_RLE8_MMTF_CHECKPOINT 4
typedef struct hsrle_rle8_mmtf128_checkpoints_info
{
  uint32_t version, headerBytes;               /* 1, 64 */
  uint32_t uncompressedSize, streamSize;       /* as in the stream's header */
  uint32_t checkpointRows, checkpointCount;    /* checkpointCount = (uncompressedSize / 16 - 1) / checkpointRows */
  uint64_t size;                               /* 64 + 4096 checkpointCount */
} hsrle_rle8_mmtf128_checkpoints_info_t;
uint64_t hsrle_rle8_mmtf128_checkpoints_bound(uint64_t uncompressedSize, uint32_t checkpointRows);
int hsrle_rle8_mmtf128_checkpoints_info_host(const void *pCheckpoints, uint64_t size, void *pInfo);
int hsrle_rle8_mmtf128_checkpoints_build_dev_async(const void *dStream, uint64_t streamSize, const void *dIndex, const hsrle_mono_index_info_t *indexInfo, uint32_t checkpointRows,
                                                   void *dCheckpoints, uint64_t capacity, uint64_t *dSize, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize,
                                                   void *stream);
uint64_t hsrle_rle8_mmtf128_range_workspace_size(uint64_t length, uint32_t spacingRows, uint32_t checkpointRows);
int hsrle_rle8_mmtf128_decompress_range_dev_async(const void *dStream, uint64_t streamSize, const void *dIndex, const hsrle_mono_index_info_t *indexInfo, const void *dCheckpoints,
                                                  const void *checkpointsInfo, uint64_t offset, uint64_t length, void *dOut, uint64_t outCapacity, uint32_t *dStatus,
                                                  void *dWorkspace, uint64_t workspaceSize, void *stream);
int hsrle_rle8_mmtf128_checkpoints_build_host(const void *pStream, uint64_t streamSize, const void *pIndex, uint64_t indexSize, uint32_t checkpointRows, void *pCheckpoints,
                                              uint64_t capacity, uint64_t *pSize);
int hsrle_rle8_mmtf128_decompress_range_host(const void *pStream, uint64_t streamSize, const void *pIndex, uint64_t indexSize, const void *pCheckpoints, uint64_t checkpointsSize,
                                             uint64_t offset, uint64_t length, void *pOut, uint64_t outCapacity);

/*
 * rle8_sh (src/rle_sh.c, rle.h:455-458): run-length coding with a bit stream of capped unary tokens -- one stream: u32 inSize, u32 streamSize, a body
 * of whole bytes upward from offset 8, the token bits downward from the last byte (csrc/hsrle_rle8sh.hip.h has the grammar).  Same names, arguments and
 * return values as the reference; the streams are the reference's byte for byte.
 * bounds: 0 above 2^30, else size + 13, the reference's value.  It is NOT an upper bound of the stream: random bytes of n >= 8 give n + 18 (the
 * reference's own test is outSize >= n + 8, and with a buffer of exactly n + 13 its bit stream and its body run into each other).
 * compress: the stream's size; 0 for a NULL pointer, inSize == 0, outSize < inSize + 8 (the reference's test).
 * decompress: the header's inSize; 0 for a NULL pointer, a zero size, header sizes larger than the arguments.  Where this library differs, on purpose:
 *  - compress returns 0 for inSize > 2^30, and 0 when the stream does not fit in outSize: it never writes past outSize.
 *  - A CAPACITY THAT ALWAYS SUFFICES is hsrle_rle8_sh_capacity(n) = n + n / 221 + 21.  Derivation: the encoder cuts the input into blocks, each ended
 *    by an EVENT -- a run of >= 10 equal bytes that becomes the new R (7 bits + 5 bytes for >= 10 bytes: at least 4.125 bytes saved) or a run of >= 15
 *    bytes of R (a FILL: more saved).  What a block costs beyond its own bytes:
 *      raw COPY large  4.875 (7 bits + u32), only for >= 263 bytes; with its event at most + 0.75 per 273 bytes = 1 / 364 per byte
 *      raw COPY small  1.875, under 7 bytes coded as symbols at most 1.5 (a literal is 2 bits + its byte): both less than the event saves
 *      encoded copy    the 7 : 2 rule (7 r > 2 o for r bytes of R and o others) admits a span whose symbols cost r / 8 + 1.25 o < r + o, but with a
 *                      margin that can be next to nothing, and the span is cut into BLOCKS OF 416 that cost 7 bits + 1 byte each; the last block may
 *                      be as short as 162, so a span of c bytes has at most (c - 162) / 416 + 1 blocks: 1.875 (c + 254) / 416 = c / 221.9 + 1.145.
 *                      THIS is the worst case per byte; with its event 1.875 c / 416 - 2.98 < c / 221.
 *    So every block with its event grows by less than (its bytes) / 221.  The last block has no event: at most 4.875, or c / 221.9 + 1.145.  The
 *    terminator is 4.875, the header 8, the bit stream is rounded up to a byte (< 1), n / 221 is rounded down (< 1): 8 + 4.875 + 4.875 + 2 < 21.
 *    tests/test_gpu_rle8_sh.py and tests/test_rle8_sh_model.py hold it against random bytes, raw blocks of 263 bytes between runs of 10, and long
 *    spans that the 7 : 2 rule admits by one byte.
 *  - decompress checks EVERY token BEFORE anything is written and returns 0 for a malformed stream: a stream shorter than 13 bytes (header, the
 *    terminator's u32, one bit byte) or a header inSize of 0 or above 2^30; a body cursor that reaches a byte whose bits were consumed, or bits that
 *    reach a consumed body byte (a missing terminator and an encoded copy whose bits run out end here); a token whose output would pass inSize; any
 *    token but the terminator behind the last output byte (a FILL of no bytes too); a terminator with output missing.  The reference checks nothing.
 *  - Everything else decodes as the reference does: a literal equal to second / third / lastOccurred, FILL large counts through the 32-bit wrap
 *    (a stored 0xFFFFFFF2 .. 0xFFFFFFFF is a count of 0 .. 13), a gap between body and bits.
 * Host pointers, staged per device like the functions above.
 */
uint32_t rle8_sh_bounds(const uint32_t size);
uint32_t rle8_sh_compress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);
uint32_t rle8_sh_decompress(const uint8_t *pIn, const uint32_t inSize, uint8_t *pOut, const uint32_t outSize);

/*
 * The same, device resident and ENQUEUE-ONLY (nothing allocates, synchronises or reads device memory; a HIP graph can capture the calls; what has to
 * be zero is zeroed by a kernel, every other word the kernels read is written by a kernel before).  Buffers at any byte address, not overlapping;
 * dOutSize / dStatus: device words, 4-byte aligned.  dWorkspace >= hsrle_rle8_sh_workspace_size(decode, uncompressed size) bytes, contents do not matter.
 * compress: 1 <= inSize <= 2^30 and outCapacity >= inSize + 8, else HSRLE_ERR_ARGUMENT / HSRLE_ERR_CAPACITY and nothing is enqueued.  *dOutSize
 *   receives the stream's size and *dStatus HSRLE_RLE8_SH_DONE, or 0 and HSRLE_RLE8_SH_CAPACITY when the stream is larger than outCapacity (then
 *   nothing is written to dOut; hsrle_rle8_sh_capacity(inSize) suffices for every input; 0 for inSize == 0 or above 2^30).  Workspace: an item per decision
 *   (size / 5), an emission record per item and per block of an encoded copy, the bit stream before it is placed: about 11 bytes per input byte.
 *   ONE wave decides run by run and ONE lane follows second / third / lastOccurred through the bytes of the symbol stretches; the
 *   bytes of raw COPYs and FILLs are touched by whole waves only.
 * decompress: outSize is the UNCOMPRESSED size, which the caller knows (the stream's first word), 1 .. 2^30.  The header is read on the device;
 *   *dStatus receives HSRLE_RLE8_SH_DONE, or HSRLE_RLE8_SH_MALFORMED (header inSize != outSize, header streamSize > streamSize, or a chain as
 *   described above); then NOTHING has been written to dOut.  Never more than outSize bytes are written.  Workspace: a record of 16 bytes and 8 bytes
 *   of summary and state per FILL, raw COPY and stretch of symbol tokens.  A record holds at least one output byte and a hand-made stream can hold
 *   one per byte, so the size is 24 bytes per output byte (a stream from the encoder uses under a fifth of the records).
 *   ONE wave tokenises the stream (the format's first serial dependence).  second / third / lastOccurred, the second: a lane per stretch sums up its
 *   own tokens, one workgroup scans the SUMMARIES (a run of records per thread) under the guess that no literal behind S / T promotes -- true of
 *   every stream the encoder writes -- and every expanding lane proves the guess for its stretch.  A failed proof sets a device word that gates the
 *   fallback inside the same call: one lane follows the state through every L / S / T token and the stretches are expanded again.
 *   For tests and measurements: behind the call, word 2 of the workspace (from its 256-byte aligned start) is 1 if the fallback ran, word 3 the
 *   number of stretches whose proof failed.
 * hsrle_rle8_sh_tuning: symbols per stretch record of the decoder (1 .. 4096; 0 or above 4096 = 128; a record is never cut inside a word of the bit
 * stream, so below 64 every word is a record of its own, of up to 64 symbols), bytes per window of its walk (64 .. 1024 in steps of 16; anything
 * else = 1024), and serialState != 0: the fallback instead of the scan, always.  Any value gives the same bytes.  PROCESS-GLOBAL, for tests.
 */
#define HSRLE_RLE8_SH_DONE 0
#define HSRLE_RLE8_SH_MALFORMED 1
#define HSRLE_RLE8_SH_CAPACITY 2
uint64_t hsrle_rle8_sh_workspace_size(int decode, uint64_t size);
uint64_t hsrle_rle8_sh_capacity(uint64_t inSize);
int hsrle_rle8_sh_compress_dev_async(const void *dIn, uint64_t inSize, void *dOut, uint64_t outCapacity, uint32_t *dOutSize, uint32_t *dStatus, void *dWorkspace,
                                     uint64_t workspaceSize, void *stream);
int hsrle_rle8_sh_decompress_dev_async(const void *dStream, uint64_t streamSize, void *dOut, uint64_t outSize, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize,
                                       void *stream);
void hsrle_rle8_sh_tuning(uint32_t stretchSymbols, uint32_t walkWindow, uint32_t serialState);

/*
 * The rle8_sh BLOCK CONTAINER: many independent rle8_sh streams per call -- the throughput path of the codec.  The input is cut into blocks of
 * blockSize bytes and block stream i is EXACTLY what rle8_sh_compress returns for input bytes [i B, min((i + 1) B, n)), its own 8-byte header
 * included; with thousands of blocks in flight the passes that are one wave or one lane inside a stream stop being serial on the device, and a
 * caller can shard the container and decode it by block range.  All fields little endian:
 *   [ 0] char     magic[8] = "HSRLESHB"
 *   [ 8] uint32_t version  = 1
 *   [12] uint32_t reserved = 0
 *   [16] uint64_t uncompressedSize
 *   [24] uint32_t blockSize      (a multiple of 128, 128 .. 2^20; the last block may be shorter)
 *   [28] uint32_t blockCount     = ceil(uncompressedSize / blockSize)
 *   [32] uint64_t payloadSize
 *   [40] uint64_t totalSize      = 64 + 8 * (blockCount + 1) + payloadSize + 32
 *   [48] uint8_t  zero[16]
 *   [64] uint64_t offset[blockCount + 1]   relative to the payload start; offset[0] = 0, offset[blockCount] = payloadSize
 *        payload: the block streams back to back, at any byte address
 *        32 zero bytes
 * It is not a section-2 container (HSRLE_CODEC_COUNT stays what it is): hsrle_container_info_host refuses this magic and the info functions here
 * refuse "HSRLEKIT".  blockSize 0 means 4096 everywhere.
 * bound: header + table + the sum of hsrle_rle8_sh_capacity(bytes of block i) + 32: always suffices.  0 for a bad block size, inSize == 0 or a block
 *   count that does not fit 32 bits.
 * workspace_size: a function of min(blocks, blocks in flight) and blockSize, NOT of inSize: blocks go through the passes in groups, each block of a
 *   group in a slot that is the workspace of a single stream of blockSize bytes (about 11 bytes per input byte to encode, 24 per output byte to
 *   decode).  A decode of a block range needs the size for (blocks of the range) * blockSize bytes.  0 where bound is 0.
 * info_host / info_dev: HSRLE_ERR_ARGUMENT for a null pointer or fewer than 64 bytes, HSRLE_ERR_FORMAT for a header that breaks any line above or
 *   a totalSize above containerSize.  info_dev reads the header from the device and synchronises the stream, like hsrle_container_info_dev.
 * The two _dev_async calls are ENQUEUE-ONLY like the single-stream calls above: nothing allocates, synchronises or reads device memory, a HIP graph
 *   can capture them; what has to be zero is zeroed by a kernel, every word a kernel reads was written by a kernel before, workspace contents do
 *   not matter.  Buffers at any byte address, not overlapping; dOutSize: a device word, 8-byte aligned; dStatus: a device word, 4-byte aligned.
 *   Refused on the host before anything is enqueued: a null pointer, a bad block size, inSize == 0, overlapping buffers, misaligned words, an info
 *   whose fields contradict each other, a block range outside the container or of no blocks (HSRLE_ERR_ARGUMENT); a workspace too small, an
 *   outCapacity under header + table + pad (compress) or under uncompressedSize (decompress) (HSRLE_ERR_CAPACITY).
 * compress: *dOutSize receives totalSize and *dStatus HSRLE_RLE8_SH_DONE; the container is complete, header included, and nothing is written at or
 *   beyond totalSize.  If the container does not fit outCapacity: HSRLE_RLE8_SH_CAPACITY, *dOutSize 0, the first 8 bytes of dOut are not the magic,
 *   nothing is written at or beyond outCapacity and what lies inside it is unspecified (the groups in front of the one that did not fit have
 *   written their streams).  The block streams are written straight to their final address: there is no staging copy of the payload.
 * decompress: decodes blocks [firstBlock, firstBlock + blockCount) into dOut + firstBlock * blockSize (the section-2 convention).  The offset table
 *   is read on the device and trusted in nothing: an entry is bad when offset[i] > offset[i + 1] or offset[i + 1] > payloadSize.  A block is
 *   MALFORMED when its entry is bad or its stream is, by every refusal rule of hsrle_rle8_sh_decompress_dev_async with the block's own
 *   uncompressed size and its entry's length as the stream size; NONE of its output bytes is written, the other blocks are decoded, and *dStatus
 *   receives HSRLE_RLE8_SH_MALFORMED if any block was, else HSRLE_RLE8_SH_DONE.  Never a byte outside the decoded range of dOut is written.
 *   The symbol state of a block is followed by one lane (the serial pass of the single-stream decoder; a block has few records); stretchSymbols
 *   and walkWindow of hsrle_rle8_sh_tuning are honoured, serialState has nothing to choose here.
 * The _host calls stage host buffers per device like the functions above: HSRLE_OK / HSRLE_ERR_*; a malformed block is HSRLE_ERR_FORMAT.
 * hsrle_rle8_sh_blocks_tuning: blocks in flight (0 = the default: 32 MiB of input per group, at least 256 and at most 8192 blocks -- DESIGN.md 4.9).
 *   Any value gives the same bytes.  PROCESS-GLOBAL, for tests.
 * BOTH block containers of this section (this one and the rle8_mmtf128 block container below) share hsrle_rle8_sh_blocks_info_t: the fields are the same.
 */
typedef struct hsrle_rle8_sh_blocks_info
{
  uint64_t uncompressedSize;
  uint32_t blockSize, blockCount;
  uint64_t payloadSize, totalSize;
} hsrle_rle8_sh_blocks_info_t;
uint64_t hsrle_rle8_sh_blocks_bound(uint64_t inSize, uint32_t blockSize);
uint64_t hsrle_rle8_sh_blocks_workspace_size(int decode, uint64_t inSize, uint32_t blockSize);
int hsrle_rle8_sh_blocks_info_host(const void *pContainer, uint64_t containerSize, hsrle_rle8_sh_blocks_info_t *pInfo);
int hsrle_rle8_sh_blocks_info_dev(const void *dContainer, uint64_t containerSize, hsrle_rle8_sh_blocks_info_t *pInfo, void *stream);
int hsrle_rle8_sh_compress_blocks_dev_async(const void *dIn, uint64_t inSize, uint32_t blockSize, void *dOut, uint64_t outCapacity, uint64_t *dOutSize, uint32_t *dStatus,
                                            void *dWorkspace, uint64_t workspaceSize, void *stream);
int hsrle_rle8_sh_decompress_blocks_dev_async(const void *dContainer, const hsrle_rle8_sh_blocks_info_t *info, uint32_t firstBlock, uint32_t blockCount, void *dOut,
                                              uint64_t outCapacity, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize, void *stream);
int hsrle_rle8_sh_compress_blocks_host(const void *pIn, uint64_t inSize, uint32_t blockSize, void *pOut, uint64_t outCapacity, uint64_t *pContainerSize);
int hsrle_rle8_sh_decompress_blocks_host(const void *pContainer, uint64_t containerSize, void *pOut, uint64_t outCapacity, uint64_t *pUncompressedSize);
void hsrle_rle8_sh_blocks_tuning(uint32_t blocksInFlight);

/*
 * The rle8_mmtf128 BLOCK CONTAINER: many independent rle8_mmtf128 streams per call -- the throughput path of that codec.  The layout is the rle8_sh block
 * container's, field for field, under the magic "HSRLEMFB", version 1: 64 header bytes, uint64_t offset[blockCount + 1] relative to the payload, the
 * block streams back to back at any byte address, 32 zero bytes; the info struct is hsrle_rle8_sh_blocks_info_t itself.  Block stream i is EXACTLY what
 * this library's rle8_mmtf128_compress returns for input bytes [i B, min((i + 1) B, n)), its own 8-byte header included: the first packet's start
 * value is zero and the move-to-front lists are the IDENTITY at the start of every block.  Only the last block can have size % 16 tail ranks; it may be
 * shorter than 16 bytes, and then has no rows: a first COPY 0x06, the terminator, the tail.  With the lists restarted the transform of a block needs no
 * state table and no scan, the span scan of a block is one wave's work and every block's header chain is walked by a wave of its own: none of the
 * single stream's serial passes is left.  The restart costs ratio: every block pays again for bringing its symbols to the front of its lists.
 * Each family's info functions refuse the other two magics ("HSRLEKIT", "HSRLESHB", "HSRLEMFB").  blockSize: a multiple of 128, 128 .. 2^20; 0 means 4096.
 * bound: header + table + the sum of (bytes of block i + 13) + 32: always suffices (inSize + 13 suffices for one stream, see above).  0 for a bad block
 *   size, inSize == 0 or a block count that does not fit 32 bits.
 * workspace_size: a function of min(blocks, blocks in flight) and blockSize, NOT of inSize: a slot per block in flight -- its rank buffer (blockSize + 16),
 *   and 32 bytes per span of 64 rows (compress) or 16 bytes per row for the packet records (decompress).  A decode of a block range needs the size
 *   for (blocks of the range) * blockSize bytes.  0 where bound is 0.
 * info_host / info_dev, the refusals of the two ENQUEUE-ONLY _dev_async calls and their order, the _host calls and their return values: as for the
 *   rle8_sh block container above, word for word (a null pointer, a bad block size, inSize == 0, overlapping buffers, misaligned words, an info whose
 *   fields contradict each other, a block range outside the container or of no blocks: HSRLE_ERR_ARGUMENT; a workspace too small, an outCapacity
 *   under header + table + pad (compress) or under uncompressedSize (decompress): HSRLE_ERR_CAPACITY).  Nothing allocates, synchronises or reads
 *   device memory; a HIP graph can capture the calls as a linear chain; every word a kernel reads was written by a kernel of the same call; workspace
 *   contents do not matter; buffers at any byte address.  The status words are HSRLE_RLE8_MMTF_DONE / _MALFORMED / _CAPACITY.
 * compress: *dOutSize receives totalSize and *dStatus HSRLE_RLE8_MMTF_DONE; the container is complete and written straight to its final address,
 *   nothing at or beyond totalSize.  If it does not fit outCapacity: HSRLE_RLE8_MMTF_CAPACITY, *dOutSize 0, the first 8 bytes of dOut are not the
 *   magic, nothing is written at or beyond outCapacity and what lies inside it is unspecified.
 * decompress: decodes blocks [firstBlock, firstBlock + blockCount) into dOut + firstBlock * blockSize.  The offset table is trusted in nothing.  A block
 *   is MALFORMED when its entry is bad (offset[i] > offset[i + 1] or offset[i + 1] > payloadSize) or its stream breaks any refusal rule of
 *   hsrle_rle8_mmtf128_decompress_dev_async, applied with the block's own size and its entry's length; NONE of its output bytes is written (the walk's
 *   verdict gates the block's expansion and its inverse transform), the other blocks are decoded, and *dStatus receives HSRLE_RLE8_MMTF_MALFORMED
 *   if any block was.  Never a byte outside the decoded range of dOut is written.
 * hsrle_rle8_mmtf128_blocks_tuning: blocks in flight (0 = the default of the rle8_sh block container).  hsrle_rle8_mmtf_tuning (rows per span) is
 *   honoured by the per-block compress passes and changes the compress workspace; hsrle_mmtf_tuning has nothing to choose here: the segment is the
 *   block.  Any value gives the same bytes.  PROCESS-GLOBAL, for tests.
 */
uint64_t hsrle_rle8_mmtf128_blocks_bound(uint64_t inSize, uint32_t blockSize);
uint64_t hsrle_rle8_mmtf128_blocks_workspace_size(int decode, uint64_t inSize, uint32_t blockSize);
int hsrle_rle8_mmtf128_blocks_info_host(const void *pContainer, uint64_t containerSize, hsrle_rle8_sh_blocks_info_t *pInfo);
int hsrle_rle8_mmtf128_blocks_info_dev(const void *dContainer, uint64_t containerSize, hsrle_rle8_sh_blocks_info_t *pInfo, void *stream);
int hsrle_rle8_mmtf128_compress_blocks_dev_async(const void *dIn, uint64_t inSize, uint32_t blockSize, void *dOut, uint64_t outCapacity, uint64_t *dOutSize, uint32_t *dStatus,
                                                 void *dWorkspace, uint64_t workspaceSize, void *stream);
int hsrle_rle8_mmtf128_decompress_blocks_dev_async(const void *dContainer, const hsrle_rle8_sh_blocks_info_t *info, uint32_t firstBlock, uint32_t blockCount, void *dOut,
                                                   uint64_t outCapacity, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize, void *stream);
int hsrle_rle8_mmtf128_compress_blocks_host(const void *pIn, uint64_t inSize, uint32_t blockSize, void *pOut, uint64_t outCapacity, uint64_t *pContainerSize);
int hsrle_rle8_mmtf128_decompress_blocks_host(const void *pContainer, uint64_t containerSize, void *pOut, uint64_t outCapacity, uint64_t *pUncompressedSize);
void hsrle_rle8_mmtf128_blocks_tuning(uint32_t blocksInFlight);

int hsrle_kernel_waves_per_cu(int codec, int decode);
const char *hsrle_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HSRLE_H */
