// hsrle_capi_host.h -- part of hsrle_capi.hip: launch tables, the size helpers every plan uses, the small rules of every entry point, per-device state and
// scratch pool, the drop-in calls' staging and their one staged trip, the device entry and the host-pointer bodies the single-stream codecs share
#pragma once
#include "../../include/hsrle.h"
#include "hsrle_common.hip.h"
#include "hsrle_launch.h"
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <mutex>

namespace hsrle {

static CodecLaunch g_launch[kCodecCount];   // [codec id]: every launcher of the codec (hsrle_launch.h); zero = the codec has none of that kind
static std::once_flag g_tableOnce;

static void init_tables()
{
  std::call_once(g_tableOnce, [] {
    for (auto reg : { register_w8, register_w16, register_w24, register_w32, register_w48, register_w64, register_w128, register_pp8, register_pp8s, register_pp128, register_ppL,
                      register_ppS, register_pp8w, register_ppLw, register_ppSw })
      reg(g_launch);
  });
}

static inline uint32_t bounds32(uint32_t n) { return (n > (1u << 30)) ? 0u : n + (16 + 4 + 1 + 4 + 1 + 64) * 2 + (3 * 4) + 1; }
static inline uint32_t slot_stride(uint32_t B) { return (bounds32(B) + 15u) & ~15u; }
static inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }   // (the one round-up: every workspace part is align_up(bytes, 256))

// The small rules of the entry points, once each
static inline bool ranges_overlap(const void *p, uint64_t pn, const void *q, uint64_t qn)
{
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qn && b < a + pn;
}
static inline uint8_t *workspace_start(void *dWorkspace) { return (uint8_t *)(((uintptr_t)dWorkspace + 255u) & ~(uintptr_t)255u); }   // a caller's workspace starts at its first 256-byte line
static inline bool word_aligned(const void *dWord, uint32_t bytes) { return ((uintptr_t)dWord & (bytes - 1u)) == 0u; }                  // a size or status word of 4 or 8 bytes
static inline uint32_t clamp32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

static uint32_t env_u32(const char *name, uint32_t dflt) { return knob_u32(name, dflt); }   // (developer knobs: -DHSRLE_EXPERIMENTS builds only, hsrle_launch.h)
static uint32_t pow2_floor(uint64_t v) { uint32_t r = 1; while ((uint64_t)r * 2u <= v && r < 0x80000000u) r *= 2u; return r; }

// ------------------------------------------------------------------------------------------------------------------
// device state

// Per DEVICE (hipGetDevice() of the calling thread): the staging buffers of the host-pointer drop-in functions.  A drop-in call holds
// the device's mutex from its first copy to its last, so concurrent drop-in calls on one device run one after the other (the reference's
// own callers are single threaded: src/main.c, src/rle_fuzz.c); calls on different devices do not meet.  The device-pointer API keeps NO
// library-owned state between calls: what it needs beyond the caller's buffers is allocated stream-ordered (hipMallocAsync on the
// caller's stream) for the duration of the call.
constexpr int kMaxDevices = 64;
enum WsKind { kCodecWs, kMonoWs };   // which drop-in workspace: rle8m and low-entropy share DeviceState::ws, the monolithic codecs have monoWs (peak device memory: the larger, not the sum)
struct DeviceState
{
  std::mutex mu;
  void *ws = nullptr, *monoWs = nullptr;   // drop-in workspaces (WsKind)
  uint64_t wsSize = 0, monoWsSize = 0;
  hipStream_t aux = nullptr;   // second stream of the chunked compression
  hipMemPool_t pool = nullptr; // the library's OWN stream-ordered pool on this device (scratch_alloc): the application's default pool is never touched
  bool poolTried = false;
  void *monoIn = nullptr, *monoOut = nullptr, *monoAux = nullptr; // staging of the drop-in (host pointer) path
  uint64_t monoInSize = 0, monoOutSize = 0;
};

static DeviceState g_devs[kMaxDevices];
static std::once_flag g_deviceOnce;
static int g_deviceCount = 0;

static bool device_ok()
{
  std::call_once(g_deviceOnce, [] {
    int n = 0;
    g_deviceCount = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? n : 0;
  });
  return g_deviceCount > 0;
}

static DeviceState &this_device()
{
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices) d = 0;
  return g_devs[d];
}

// Scratch for the duration of one call on `st`: stream-ordered, so concurrent calls on other streams (or threads) never share it.  It
// comes from a pool the LIBRARY owns (one per device, created on first use): freed scratch stays in that pool up to the retention set
// with hsrle_scratch_retention() (default 2 GiB: the small per-call scratch of decode / info calls is never given back and re-mapped;
// the 9 GB workspace of an 8 GiB compression without a caller's workspace is) and hsrle_trim() hands all of it back.  Round 2 raised the
// release threshold of the device's DEFAULT pool instead, which kept gigabytes away from the host application's own allocator.
static std::atomic<uint64_t> g_scratchRetention{ 2ull << 30 };
static hipMemPool_t device_pool()
{
  DeviceState &D = this_device();
  std::lock_guard<std::mutex> lock(D.mu);
  if (!D.poolTried)
  {
    D.poolTried = true;
    int d = 0;
    hipMemPoolProps props = {};
    props.allocType = hipMemAllocationTypePinned;
    props.handleTypes = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = (hipGetDevice(&d) == hipSuccess) ? d : 0;
    hipMemPool_t pool = nullptr;
    if (hipMemPoolCreate(&pool, &props) == hipSuccess)
    {
      uint64_t keep = g_scratchRetention.load();
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
      D.pool = pool;
    }
    else
      (void)hipGetLastError();
  }
  return D.pool;
}
static void *scratch_alloc(uint64_t bytes, hipStream_t st)
{
  void *p = nullptr;
  hipMemPool_t pool = device_pool();
  if (pool != nullptr && hipMallocFromPoolAsync(&p, bytes, pool, st) == hipSuccess) return p;
  (void)hipGetLastError();
  if (hipMallocAsync(&p, bytes, st) == hipSuccess) return p;           // (no pool of our own on this runtime: the default pool, untouched)
  (void)hipGetLastError();
  return nullptr;
}
static void scratch_free(void *p, hipStream_t st) { if (p) (void)hipFreeAsync(p, st); }

static bool grow(void **p, uint64_t *have, uint64_t need)
{
  if (*have >= need && *p)
    return true;
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  *have = 0;
  if (hipMalloc(p, need) != hipSuccess)
    return false;
  *have = need;
  return true;
}

// One host-pointer drop-in call (hsrle_capi_dropin.h): holds the device's mutex from its construction -- in front of the first copy -- to the end of the
// call, and hands out the device's staging buffers.  Every family stages through this one sequence: reserve, copy up, enqueue, read words, copy down.
// (hsrle_compress_host / hsrle_decompress_host allocate and free per call: another contract, not staged here.)
struct Staging
{
  DeviceState &D;
  std::lock_guard<std::mutex> lock;
  uint8_t *in = nullptr, *out = nullptr, *ws = nullptr;
  uint64_t wsSize = 0;
  uint32_t *status = nullptr;          // the device's status words (256 bytes, allocated with the first call's buffers; the words at + 64)

  Staging() : D(this_device()), lock(D.mu) {}

  // input and output buffers of at least these sizes (outBytes 0: the call has no output).  The input gets 256 bytes more -- the decoders' 128-byte
  // zero tail and their reads up to C + 64 live there --, the output 64.
  bool reserve(uint64_t inBytes, uint64_t outBytes)
  {
    if (!grow(&D.monoIn, &D.monoInSize, inBytes + 256) || (outBytes && !grow(&D.monoOut, &D.monoOutSize, outBytes + 64)) || (!D.monoAux && hipMalloc(&D.monoAux, 256) != hipSuccess))
      return false;
    in = (uint8_t *)D.monoIn; out = (uint8_t *)D.monoOut; status = (uint32_t *)((uint8_t *)D.monoAux + 64);
    return true;
  }
  bool reserve_ws(uint64_t bytes, WsKind kind = kCodecWs)
  {
    void **p = kind == kMonoWs ? &D.monoWs : &D.ws;
    uint64_t *have = kind == kMonoWs ? &D.monoWsSize : &D.wsSize;
    if (!grow(p, have, bytes))
      return false;
    ws = (uint8_t *)*p; wsSize = *have;
    return true;
  }
  // n host bytes to in + at, zeroTail zero bytes behind them
  bool up(const void *p, uint64_t n, uint64_t at = 0, uint32_t zeroTail = 0)
  {
    return (n == 0 || hipMemcpy(in + at, p, n, hipMemcpyHostToDevice) == hipSuccess) && (zeroTail == 0 || hipMemset(in + at + n, 0, zeroTail) == hipSuccess);
  }
  bool words(uint32_t *to, const void *dFrom, uint32_t count) { return hipMemcpy(to, dFrom, 4ull * count, hipMemcpyDeviceToHost) == hipSuccess; }
  bool down(void *to, const void *dFrom, uint64_t n) { return hipMemcpy(to, dFrom, n, hipMemcpyDeviceToHost) == hipSuccess; }
};

// The staged trip of a host-pointer call whose verdict is in its status words: reserve, copy up, enqueue(s) -> HSRLE_* code, read `wordCount` status words
// (0: the call has none), judge(words, n) -> HSRLE_* code and the bytes to hand back, copy them down.  Returns how far it got as a code: HSRLE_ERR_DEVICE for
// a reservation or copy that failed, else the first code of enqueue / judge that is not HSRLE_OK, else HSRLE_OK with *copied bytes in pOut.
// inExtra: input staging behind the inBytes, for a second input that enqueue copies up itself (Staging::up with an offset).
template <typename Enqueue, typename Judge>
static int staged_call(const void *pIn, uint64_t inBytes, uint64_t outBytes, uint64_t wsBytes, void *pOut, uint32_t wordCount, Enqueue enqueue, Judge judge, uint64_t *copied,
                       uint64_t inExtra = 0)
{
  Staging s;
  if (!s.reserve(inBytes + inExtra, outBytes) || !s.reserve_ws(wsBytes) || !s.up(pIn, inBytes))
    return HSRLE_ERR_DEVICE;
  int rc = enqueue(s);
  if (rc != HSRLE_OK)
    return rc;
  uint32_t h[4] = { 0u, 0u, 0u, 0u };
  if (wordCount != 0u && !s.words(h, s.status, wordCount))
    return HSRLE_ERR_DEVICE;
  uint64_t n = 0;
  if ((rc = judge(h, n)) != HSRLE_OK)
    return rc;
  if (!s.down(pOut, s.out, n))                                           // (the copy synchronises the null stream)
    return HSRLE_ERR_DEVICE;
  *copied = n;
  return HSRLE_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// the single-stream codecs (rle8_sh: hsrle_capi_sh.h, rle8_mmtf128: hsrle_capi_mmtf.h): one device entry, one host-pointer body, per direction

// The check order of both directions: a null pointer or no plan -> ARGUMENT; overlap or a misaligned word -> ARGUMENT; output or workspace too small -> CAPACITY.
// (the checks alone, with the plan they made: the indexed calls of rle8_mmtf128 put their own between them and the enqueue)
template <typename Plan, typename PlanFn>
static int stream_compress_check(PlanFn plan, const void *dIn, uint64_t inSize, void *dOut, uint64_t outCapacity, uint32_t *dOutSize, uint32_t *dStatus, void *dWorkspace,
                                 uint64_t workspaceSize, Plan &p)
{
  if (dIn == nullptr || dOut == nullptr || dOutSize == nullptr || dStatus == nullptr || dWorkspace == nullptr || !plan(inSize, p))
    return HSRLE_ERR_ARGUMENT;
  if (ranges_overlap(dIn, inSize, dOut, outCapacity) || !word_aligned(dOutSize, 4) || !word_aligned(dStatus, 4))
    return HSRLE_ERR_ARGUMENT;
  if (outCapacity < inSize + 8u || workspaceSize < p.total)
    return HSRLE_ERR_CAPACITY;
  return HSRLE_OK;
}

template <typename Plan, typename PlanFn>
static int stream_compress_entry(PlanFn plan, hipError_t (*enqueue)(const Plan &, const uint8_t *, uint8_t *, uint32_t, uint32_t *, uint32_t *, uint8_t *, hipStream_t), const void *dIn,
                                 uint64_t inSize, void *dOut, uint64_t outCapacity, uint32_t *dOutSize, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize, void *stream)
{
  Plan p;
  const int rc = stream_compress_check(plan, dIn, inSize, dOut, outCapacity, dOutSize, dStatus, dWorkspace, workspaceSize, p);
  if (rc != HSRLE_OK)
    return rc;
  return enqueue(p, (const uint8_t *)dIn, (uint8_t *)dOut, clamp32(outCapacity), dOutSize, dStatus, workspace_start(dWorkspace), (hipStream_t)stream) == hipSuccess ? HSRLE_OK
                                                                                                                                                                  : HSRLE_ERR_DEVICE;
}

template <typename Plan, typename PlanFn>
static int stream_decompress_check(PlanFn plan, const void *dStream, uint64_t streamSize, void *dOut, uint64_t outSize, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize,
                                   Plan &p)
{
  if (dStream == nullptr || dOut == nullptr || dStatus == nullptr || dWorkspace == nullptr || streamSize == 0u || !plan(outSize, p))
    return HSRLE_ERR_ARGUMENT;
  if (ranges_overlap(dStream, streamSize, dOut, outSize) || !word_aligned(dStatus, 4))
    return HSRLE_ERR_ARGUMENT;
  if (workspaceSize < p.total)
    return HSRLE_ERR_CAPACITY;
  return HSRLE_OK;
}

template <typename Plan, typename PlanFn>
static int stream_decompress_entry(PlanFn plan, hipError_t (*enqueue)(const Plan &, const uint8_t *, uint32_t, uint8_t *, uint32_t *, uint8_t *, hipStream_t), const void *dStream,
                                   uint64_t streamSize, void *dOut, uint64_t outSize, uint32_t *dStatus, void *dWorkspace, uint64_t workspaceSize, void *stream)
{
  Plan p;
  const int rc = stream_decompress_check(plan, dStream, streamSize, dOut, outSize, dStatus, dWorkspace, workspaceSize, p);
  if (rc != HSRLE_OK)
    return rc;
  return enqueue(p, (const uint8_t *)dStream, clamp32(streamSize), (uint8_t *)dOut, dStatus, workspace_start(dWorkspace), (hipStream_t)stream) == hipSuccess ? HSRLE_OK : HSRLE_ERR_DEVICE;
}

// What the reference-named host-pointer pair of such a codec is made of: its device entries, the largest input, the smallest legal stream, the DONE word
struct StreamCodec
{
  uint64_t (*workspaceSize)(int decode, uint64_t size);
  int (*compress)(const void *, uint64_t, void *, uint64_t, uint32_t *, uint32_t *, void *, uint64_t, void *);
  int (*decompress)(const void *, uint64_t, void *, uint64_t, uint32_t *, void *, uint64_t, void *);
  uint32_t maxIn, minStream, done;
};

// outReserve: bytes of staging output; deviceCapacity: what the device entry is told it may write (both codecs' own functions of inSize).  Size and status
// word of the call: Staging::status.
static uint32_t stream_compress_dropin(const StreamCodec &c, uint64_t outReserve, uint64_t deviceCapacity, const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize)
{
  if (pIn == nullptr || pOut == nullptr || inSize == 0u || inSize > c.maxIn || outSize < inSize + 8u)   // (the reference's own test: rle8_mmtf128_compress_bounds)
    return 0;
  const uint64_t need = c.workspaceSize(0, inSize);
  if (need == 0u || !device_ok())
    return 0;
  uint64_t size = 0;
  const int rc = staged_call(
    pIn, inSize, outReserve, need, pOut, 2u, [&](Staging &s) { return c.compress(s.in, inSize, s.out, deviceCapacity, s.status, s.status + 1, s.ws, s.wsSize, nullptr); },
    [&](const uint32_t *h, uint64_t &n) { n = h[0]; return h[1] != c.done || h[0] == 0u || h[0] > outSize ? HSRLE_ERR_DEVICE : HSRLE_OK; }, &size);   // h: size, status
  return rc == HSRLE_OK ? (uint32_t)size : 0u;
}

static uint32_t stream_decompress_dropin(const StreamCodec &c, const uint8_t *pIn, uint32_t inSize, uint8_t *pOut, uint32_t outSize)
{
  if (pIn == nullptr || pOut == nullptr || inSize < 8u || outSize == 0u)
    return 0;
  uint32_t hdr[2];
  memcpy(hdr, pIn, 8);
  const uint32_t expectedOut = hdr[0], expectedIn = hdr[1];
  if (expectedOut > outSize || expectedIn > inSize || expectedOut == 0u || expectedOut > c.maxIn || expectedIn < c.minStream)
    return 0;
  const uint64_t need = c.workspaceSize(1, expectedOut);
  if (need == 0u || !device_ok())
    return 0;
  uint64_t size = 0;
  const int rc = staged_call(
    pIn, expectedIn, expectedOut, need, pOut, 1u, [&](Staging &s) { return c.decompress(s.in, expectedIn, s.out, expectedOut, s.status, s.ws, s.wsSize, nullptr); },
    [&](const uint32_t *h, uint64_t &n) { n = expectedOut; return h[0] != c.done ? HSRLE_ERR_DEVICE : HSRLE_OK; }, &size);
  return rc == HSRLE_OK ? expectedOut : 0u;
}

} // namespace hsrle
