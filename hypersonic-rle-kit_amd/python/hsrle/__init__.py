"""hsrle -- thin ctypes binding of libhsrle_hip.so (include/hsrle.h) for tests, bench.py and the multi-GPU driver.

PyTorch is used only as plumbing: device allocations (uint8 tensors), streams and torch.distributed.  Every codec call goes
through the C ABI into the hand-written gfx950 kernels; there is no Python or CPU implementation behind this module -- if the
shared library is missing or no GPU is present the calls raise.

The codec table mirrors the reference's plugin table (reference: src/codec_funcs.h:262-410): `CODECS[i]` is the name of the
(compress, decompress) pair with id i, e.g. "rle8_packed_multi", "rle64_3symlut_byte".
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.dirname(os.path.dirname(_HERE))
LIB_PATH = os.environ.get("HSRLE_LIB", os.path.join(PKG_DIR, "libhsrle_hip.so"))  # HSRLE_LIB: developer override for A/B builds

OK, ERR_ARGUMENT, ERR_CAPACITY, ERR_FORMAT, ERR_DEVICE, ERR_UNSUPPORTED = range(6)
SYNTH_RUNS, SYNTH_VIDEO = 0, 1
DEFAULT_BLOCK_SIZE = 4096
HEADER_SIZE = 64
TAIL_PAD = 32


class HsrleError(RuntimeError):
    def __init__(self, status, what):
        self.status = status
        super().__init__(f"{what}: {_lib().hsrle_status_string(status).decode()} ({status})")


class ContainerInfo(ctypes.Structure):
    _fields_ = [
        ("version", ctypes.c_uint32),
        ("codec", ctypes.c_uint32),
        ("uncompressedSize", ctypes.c_uint64),
        ("blockSize", ctypes.c_uint32),
        ("blockCount", ctypes.c_uint32),
        ("payloadSize", ctypes.c_uint64),
        ("totalSize", ctypes.c_uint64),
    ]

    @property
    def payload_start(self):
        return HEADER_SIZE + 8 * (self.blockCount + 1)


class Rle8ShBlocksInfo(ctypes.Structure):
    """hsrle_rle8_sh_blocks_info_t: the header of an rle8_sh block container, and of an rle8_mmtf128 block container (the fields are the same)."""

    _fields_ = [
        ("uncompressedSize", ctypes.c_uint64),
        ("blockSize", ctypes.c_uint32),
        ("blockCount", ctypes.c_uint32),
        ("payloadSize", ctypes.c_uint64),
        ("totalSize", ctypes.c_uint64),
    ]

    @property
    def payload_start(self):
        return HEADER_SIZE + 8 * (self.blockCount + 1)


class MonoIndexInfo(ctypes.Structure):
    """hsrle_mono_index_info_t: the header of a persistent index of one monolithic stream."""

    _fields_ = [
        ("version", ctypes.c_uint32),
        ("codec", ctypes.c_uint32),
        ("uncompressedSize", ctypes.c_uint32),
        ("compressedSize", ctypes.c_uint32),
        ("spacing", ctypes.c_uint32),
        ("recordCount", ctypes.c_uint32),
        ("recordBytes", ctypes.c_uint32),
        ("streamHead", ctypes.c_uint8 * 16),
        ("indexBytes", ctypes.c_uint64),
    ]


class Rle8mInfo(ctypes.Structure):
    """hsrle_rle8m_info_t: the header fields of an rle8m stream."""

    _fields_ = [("compressedSize", ctypes.c_uint32), ("uncompressedSize", ctypes.c_uint32), ("sections", ctypes.c_uint32)]


# ----------------------------------------------------------------------------------------------------------------------
# the signatures of include/hsrle.h as data: symbol -> (restype, argtypes).  tests/test_binding_signatures.py holds them against the header's prototypes:
# a pointer to void or to an integer is c_void_p (POINTER of the integer where a caller passes byref of one), const char * is c_char_p, a pointer to one of
# the four info structs is POINTER of its class above, every other struct pointer is c_void_p, scalars are themselves.  (The checkpoint sidecar's info struct,
# Rle8MmtfCheckpointsInfo below, is declared void * in the header for that reason.)


def _signatures():
    ci, u32, u64, vp, cs, P = ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER
    kit, shb, idx, r8m = P(ContainerInfo), P(Rle8ShBlocksInfo), P(MonoIndexInfo), P(Rle8mInfo)
    stream_enc, stream_dec = (ci, [vp, u64, vp, u64, vp, vp, vp, u64, vp]), (ci, [vp, u64, vp, u64, vp, vp, u64, vp])
    table = {
        "hsrle_codec_from_name": (ci, [cs]),
        "hsrle_codec_name": (cs, [ci]),
        "hsrle_status_string": (cs, [ci]),
        "hsrle_version": (cs, []),
        "hsrle_build_id": (cs, []),
        "hsrle_device_count": (ci, []),
        "hsrle_experiments_enabled": (ci, []),
        "hsrle_scratch_retention": (ci, [u64]),
        "hsrle_trim": (ci, []),
        "hsrle_encode_path": (ci, [ci, u64, u32]),
        "hsrle_decode_ring": (ci, [ci, u64, u64]),
        "hsrle_suggest_block_size": (u32, [u64]),
        "hsrle_kernel_waves_per_cu": (ci, [ci, ci]),
        "rle_compress_bounds": (u32, [u32]),
        "rle_decompress_additional_size": (u32, []),
        # 1. monolithic streams: host pointers, device pointers, the persistent index
        "hsrle_compress_mono": (u32, [ci, vp, u32, vp, u32]),
        "hsrle_decompress_mono": (u32, [ci, vp, u32, vp, u32]),
        "hsrle_decompress_mono_workspace_size": (u64, [ci, u32, u32]),
        "hsrle_compress_mono_workspace_size": (u64, [ci, u32]),
        "hsrle_decompress_mono_dev": (ci, [ci, vp, u32, vp, u64, vp, u64, P(u32), P(u32), vp]),
        "hsrle_decompress_mono_dev_async": (ci, [ci, vp, vp, u32, vp, u64, vp, u64, P(u32), vp, vp]),
        "hsrle_compress_mono_dev": (ci, [ci, vp, u32, vp, u64, vp, u64, P(u32), P(u32), vp]),
        "hsrle_compress_mono_dev_async": (ci, [ci, vp, u32, vp, u64, vp, u64, vp, vp]),
        "hsrle_compress_mono_dev_enqueue": (ci, [ci, vp, u32, vp, u64, vp, u64, vp, vp, vp]),
        "hsrle_mono_tuning": (None, [u32, u32, u32]),
        "hsrle_mono_encode_stats": (None, [P(u32)]),
        "hsrle_mono_index_size": (u64, [ci, u32, u32, u32]),
        "hsrle_mono_index_workspace_size": (u64, [ci, u32, u32, u32]),
        "hsrle_mono_index_build_dev": (ci, [ci, vp, u32, u32, vp, u64, vp, u64, idx, vp]),
        "hsrle_mono_index_info_host": (ci, [vp, u64, idx]),
        "hsrle_mono_decompress_range_dev_async": (ci, [vp, vp, idx, u64, u64, vp, u64, vp, vp]),
        # 2. the block container
        "hsrle_container_bound": (u64, [u64, u32]),
        "hsrle_compress_workspace_size": (u64, [u64, u32]),
        "hsrle_compress_workspace_size_codec": (u64, [ci, u64, u32]),
        "hsrle_compress_dev_async": (ci, [ci, vp, u64, vp, u64, u32, vp, u64, vp]),
        "hsrle_compress_dev": (ci, [ci, vp, u64, vp, u64, u32, P(u64), vp]),
        "hsrle_container_info_dev": (ci, [vp, u64, kit, vp]),
        "hsrle_container_info_host": (ci, [vp, u64, kit]),
        "hsrle_decompress_dev_async": (ci, [vp, kit, vp, u64, vp, vp]),
        "hsrle_decompress_blocks_dev_async": (ci, [vp, kit, u32, u32, vp, u64, vp, vp]),
        "hsrle_decompress_range_dev_async": (ci, [vp, kit, u64, u64, vp, u64, vp, vp]),
        "hsrle_decompress_dev": (ci, [vp, u64, vp, u64, P(u64), vp]),
        "hsrle_compress_host": (ci, [ci, vp, u64, vp, u64, u32, P(u64)]),
        "hsrle_decompress_host": (ci, [vp, u64, vp, u64, P(u64)]),
        "hsrle_split_sub_block_size": (u32, [kit, u32]),
        "hsrle_decompress_split_workspace_size": (u64, [kit, u32, u32]),
        "hsrle_decompress_split_dev_async": (ci, [vp, kit, u32, u32, vp, u64, vp, vp, u64, u32, vp]),
        "hsrle_hash_blocks_dev_async": (ci, [vp, kit, u32, u32, vp, vp]),
        "hsrle_synth_dev_async": (ci, [ci, ci, u64, vp, u64, vp]),
        # 4. containers across ranks
        "hsrle_rccl_unique_id": (ci, [vp]),
        "hsrle_rccl_comm_create": (ci, [vp, ci, ci, P(vp)]),
        "hsrle_rccl_comm_destroy": (ci, [vp]),
        "hsrle_rccl_comm_ranks": (ci, [vp, P(ci), P(ci)]),
        "hsrle_gather_container_rccl": (ci, [vp, ci, vp, u64, u64, vp, u64, P(u64), vp]),
        "hsrle_scatter_container_rccl": (ci, [vp, ci, vp, u64, vp, u64, P(u64), vp]),
        # rle8m and the low-entropy codec
        "rle8m_opencl_init": (ctypes.c_bool, [ctypes.c_size_t] * 3),
        "rle8m_opencl_destroy": (None, []),
        "rle8m_compress_bounds": (u32, [u32, u32]),
        "rle8m_compress": (u32, [u32, vp, u32, vp, u32]),
        "rle8_low_entropy_compress_bounds": (u32, [u32]),
        "rle8_low_entropy_short_compress_bounds": (u32, [u32]),
        "rle8_low_entropy_decompressed_size": (u32, [vp, u32]),
        "rle8_low_entropy_get_compress_info": (ctypes.c_bool, [vp, u32, vp]),
        "rle8_low_entropy_get_compress_info_only_max_frequency": (ctypes.c_bool, [vp, u32, vp]),
        "rle8_low_entropy_write_compress_info": (u32, [vp, vp, u32]),
        "rle8_low_entropy_read_decompress_info": (u32, [vp, u32, vp]),
        "rle8_low_entropy_compress_with_info": (u32, [vp, u32, vp, vp, u32]),
        "rle8_low_entropy_short_compress_with_info": (u32, [vp, u32, vp, vp, u32]),
        "rle8_low_entropy_decompress_with_info": (u32, [vp, vp, vp, vp, u32]),
        "rle8_low_entropy_short_decompress_with_info": (u32, [vp, vp, vp, vp, u32]),
        "hsrle_low_entropy_workspace_size": (u64, [u32]),
        "hsrle_low_entropy_compress_dev_async": (ci, [vp, u32, ci, vp, u64, vp, u64, vp, vp]),
        "hsrle_low_entropy_decompress_workspace_size": (u64, [u64]),
        "hsrle_low_entropy_decompress_dev": (ci, [vp, u64, vp, u64, vp, u64, vp, vp]),
        "hsrle_rle8m_compress_workspace_size": (u64, [u32, u32]),
        "hsrle_rle8m_compress_dev_async": (ci, [vp, u32, u32, vp, u64, vp, u64, vp, vp]),
        "hsrle_rle8m_info_dev": (ci, [vp, u64, r8m, vp]),
        "hsrle_rle8m_decompress_dev_async": (ci, [vp, r8m, vp, u64, vp, vp]),
        # 5. the stream codecs: the mmtf transforms, rle8_mmtf128, rle8_sh and the block containers of the two
        "hsrle_mmtf_workspace_size": (u64, [ci, u64]),
        "hsrle_mmtf_dev_async": (ci, [ci, ci, vp, u64, vp, vp, u64, vp]),
        "hsrle_mmtf_tuning": (None, [u32]),
        "hsrle_rle8_mmtf128_workspace_size": (u64, [ci, u64]),
        "hsrle_rle8_mmtf128_compress_dev_async": stream_enc,
        "hsrle_rle8_mmtf128_decompress_dev_async": stream_dec,
        "hsrle_rle8_mmtf_tuning": (None, [u32]),
        "hsrle_rle8_mmtf128_index_bound": (u64, [u64, u32]),
        "hsrle_rle8_mmtf128_index_info_host": (ci, [vp, u64, idx]),
        "hsrle_rle8_mmtf128_compress_indexed_dev_async": (ci, stream_enc[1][:-1] + [u32, vp, u64, vp, vp]),
        "hsrle_rle8_mmtf128_index_build_dev_async": (ci, [vp, u64, u64, u32, vp, u64, vp, vp, vp]),
        "hsrle_rle8_mmtf128_decompress_indexed_dev_async": (ci, [vp, u64, vp, idx, vp, u64, vp, vp, u64, vp]),
        "hsrle_rle8_mmtf128_index_build_host": (ci, [vp, u64, u32, vp, u64, P(u64)]),
        "hsrle_rle8_mmtf128_decompress_indexed_host": (ci, [vp, u64, vp, u64, vp, u64, P(u64)]),
        "hsrle_rle8_mmtf128_checkpoints_bound": (u64, [u64, u32]),
        "hsrle_rle8_mmtf128_checkpoints_info_host": (ci, [vp, u64, vp]),                    # (the info: Rle8MmtfCheckpointsInfo, through void * in the header)
        "hsrle_rle8_mmtf128_checkpoints_build_dev_async": (ci, [vp, u64, vp, idx, u32, vp, u64, vp, vp, vp, u64, vp]),
        "hsrle_rle8_mmtf128_range_workspace_size": (u64, [u64, u32, u32]),
        "hsrle_rle8_mmtf128_decompress_range_dev_async": (ci, [vp, u64, vp, idx, vp, vp, u64, u64, vp, u64, vp, vp, u64, vp]),
        "hsrle_rle8_mmtf128_checkpoints_build_host": (ci, [vp, u64, vp, u64, u32, vp, u64, P(u64)]),
        "hsrle_rle8_mmtf128_decompress_range_host": (ci, [vp, u64, vp, u64, vp, u64, u64, u64, vp, u64]),
        "hsrle_rle8_sh_workspace_size": (u64, [ci, u64]),
        "hsrle_rle8_sh_capacity": (u64, [u64]),
        "hsrle_rle8_sh_compress_dev_async": stream_enc,
        "hsrle_rle8_sh_decompress_dev_async": stream_dec,
        "hsrle_rle8_sh_tuning": (None, [u32, u32, u32]),
        "hsrle_rle8_sh_blocks_bound": (u64, [u64, u32]),
        "hsrle_rle8_sh_blocks_workspace_size": (u64, [ci, u64, u32]),
        "hsrle_rle8_sh_blocks_info_host": (ci, [vp, u64, shb]),
        "hsrle_rle8_sh_blocks_info_dev": (ci, [vp, u64, shb, vp]),
        "hsrle_rle8_sh_compress_blocks_dev_async": (ci, [vp, u64, u32, vp, u64, vp, vp, vp, u64, vp]),
        "hsrle_rle8_sh_decompress_blocks_dev_async": (ci, [vp, shb, u32, u32, vp, u64, vp, vp, u64, vp]),
        "hsrle_rle8_sh_compress_blocks_host": (ci, [vp, u64, u32, vp, u64, P(u64)]),
        "hsrle_rle8_sh_decompress_blocks_host": (ci, [vp, u64, vp, u64, P(u64)]),
        "hsrle_rle8_sh_blocks_tuning": (None, [u32]),
    }
    # the rle8_mmtf128 block container: the rle8_sh block container's calling shapes (and its info struct) under its own names
    for tail in ("blocks_bound", "blocks_workspace_size", "blocks_info_host", "blocks_info_dev", "compress_blocks_dev_async", "decompress_blocks_dev_async",
                 "compress_blocks_host", "decompress_blocks_host", "blocks_tuning"):
        table["hsrle_rle8_mmtf128_" + tail] = table["hsrle_rle8_sh_" + tail]
    for nm in ("mmtf_bounds", "bitmmtf_bounds", "rle8_mmtf128_compress_bounds", "rle8_mmtf256_compress_bounds", "rle8_sh_bounds"):
        table[nm] = (u32, [u32])
    # the rule of the reference-named host-pointer functions (src/rle.h): (pIn, inSize, pOut, outSize) -> size, 0 = failure
    widths = (16, 24, 32, 48, 64)
    pairs = ["rle8_3symlut", "rle8_7symlut", "rle8m", "rle8_low_entropy", "rle8_low_entropy_short", "rle8_mmtf128", "rle8_sh"]
    pairs += [f"rle{W}_{v}" for W in widths + (128,) for v in ("sym", "sym_packed", "byte", "byte_packed")]
    pairs += [f"rle{W}_{k}symlut_{v}" for W in widths for k in (3, 7) for v in ("sym", "byte")]
    pairs += [f"rle8_{v}_short" for v in ("multi", "single", "1symlut", "3symlut", "7symlut")]
    pairs += [f"rle{W}_{v}_short" for W in widths for v in ("sym", "byte")] + [f"rle{W}_{k}symlut_{v}_short" for W in widths for k in (1, 3, 7) for v in ("sym", "byte")]
    names = [p + d for p in pairs for d in ("_compress", "_decompress")]
    names += ["rle8_multi_compress", "rle8_single_compress", "rle8_decompress", "rle8_packed_multi_compress", "rle8_packed_single_compress", "rle8_packed_decompress"]
    names += [f"rle{W}_{k}symlut_byte_short_compress_greedy" for W in widths for k in (1, 3, 7)]
    names += [f"{t}_{d}" for t in ("mmtf128", "mmtf256", "bitmmtf8", "bitmmtf16") for d in ("encode", "decode")]
    names += ["rle8_low_entropy_compress_only_max_frequency", "rle8_low_entropy_short_compress_only_max_frequency", "rle8m_opencl_decompress"]
    names.remove("rle8m_compress")                                       # (its first argument is the section count: in the table above)
    for nm in names:
        table[nm] = (u32, [vp, u32, vp, u32])
    return table


SIGNATURES = _signatures()
EXPERIMENT_SIGNATURES = {                                                # -DHSRLE_EXPERIMENTS builds only: declared where the library has them
    "hsrle_decompress_wave_dev_async": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ContainerInfo), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                                       ctypes.c_void_p, ctypes.c_void_p]),
}


def declare(L):
    """Give every function of include/hsrle.h its restype / argtypes on the ctypes.CDLL `L` (any build of libhsrle_hip.so).  Needs nothing but ctypes:
    no torch, no device.  A function without them would take ctypes' default of int and truncate a 64 bit size without a word."""
    for name, (restype, argtypes) in SIGNATURES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    for name, (restype, argtypes) in EXPERIMENT_SIGNATURES.items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    return L


_LIB = None


def _lib():
    """Load libhsrle_hip.so (built by `make -C hypersonic-rle-kit_amd` / __graft_entry__.build()).  Fails loudly."""
    global _LIB
    if _LIB is not None:
        return _LIB
    try:
        # torch ships its own HIP runtime; load it first so that this library binds to the SAME runtime instance
        # (two runtimes in one process do not see each other's allocations)
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C {PKG_DIR}` (hipcc, gfx950); there is no fallback codec")
    _LIB = declare(ctypes.CDLL(LIB_PATH))
    return _LIB


def lib():
    return _lib()


CODEC_COUNT = 110  # 50 extreme codecs + 44 Short + 15 Greedy encoders + rle8_single_short (include/hsrle.h)


def codec_names():
    L = _lib()
    return [L.hsrle_codec_name(i).decode() for i in range(CODEC_COUNT)]


def codec_id(name_or_id):
    if isinstance(name_or_id, int):
        return name_or_id
    cid = _lib().hsrle_codec_from_name(name_or_id.encode())
    if cid < 0:
        raise KeyError(name_or_id)
    return cid


def suggest_block_size(n):
    """Block size that gives a buffer of n bytes enough blocks to fill the GPU (hsrle_suggest_block_size)."""
    return int(_lib().hsrle_suggest_block_size(n))


def build_id():
    """The library's build id: a hash of its sources and build flags (Makefile); profiles/*_traffic.json is stamped with it."""
    return _lib().hsrle_build_id().decode()


PATH_RING, PATH_SPLIT, PATH_RUN_LIST, PATH_POSITION_PARALLEL = 0, 1, 2, 3


def encode_path(codec, size, block_size):
    """Which encoder `compress` uses for `size` bytes in blocks of `block_size` (include/hsrle.h: hsrle_encode_path; needs no device): PATH_RING
    (one lane per block), PATH_SPLIT (small containers, chunks inside the blocks) or PATH_RUN_LIST (small containers, a wave per block)."""
    cid = codec if isinstance(codec, int) else codec_id(codec)
    r = int(_lib().hsrle_encode_path(cid, size, block_size))
    if r < 0:
        raise ValueError("hsrle_encode_path: bad codec, size or block size")
    return r


def decode_ring(codec, usize, payload_size):
    """Which stream ring (64 or 128 bytes per lane) the plain block decode (`decompress_async`, block ranges included) takes for a container of `codec`
    with these header fields (include/hsrle.h: hsrle_decode_ring; needs no device).  Split decode by records and range decode always use 128; `decompress`
    takes the split decode for containers of fewer than 131 072 blocks and is not what this reports."""
    cid = codec if isinstance(codec, int) else codec_id(codec)
    r = int(_lib().hsrle_decode_ring(cid, usize, payload_size))
    if r < 0:
        raise ValueError("hsrle_decode_ring: bad codec")
    return r


def experiments_enabled():
    """True for -DHSRLE_EXPERIMENTS builds (developer knobs / kernels measured slower); the shipped library returns False."""
    return bool(_lib().hsrle_experiments_enabled())


def kernel_waves_per_cu(codec, decode=True):
    """Wavefronts of the codec's decode / encode kernel resident on one CU (from the HIP runtime's occupancy calculation)."""
    return int(_lib().hsrle_kernel_waves_per_cu(codec_id(codec), 1 if decode else 0))


def compress_bounds(n):
    return _lib().rle_compress_bounds(n)


def container_bound(n, block_size=DEFAULT_BLOCK_SIZE):
    return _lib().hsrle_container_bound(n, block_size)


def workspace_size(n, block_size=DEFAULT_BLOCK_SIZE, codec=None):
    """Bytes of workspace for compress_async; with a codec (key or id): hsrle_compress_workspace_size_codec (8 bit Single / 128 bit: small containers
    then take the split encode)."""
    if codec is None:
        return _lib().hsrle_compress_workspace_size(n, block_size)
    return _lib().hsrle_compress_workspace_size_codec(codec_id(codec), n, block_size)


# ----------------------------------------------------------------------------------------------------------------------
# drop-in (host pointer, monolithic stream) path


def mono_compress(codec, data):
    """Reference-compatible single stream (what `<codec>_compress` of rle.h returns).  bytes -> bytes | None (failure)."""
    data = bytes(data)
    n = len(data)
    cap = compress_bounds(n) if n else 0
    out = ctypes.create_string_buffer(max(cap, 1))
    size = _lib().hsrle_compress_mono(codec_id(codec), data, n, out, cap)
    return out.raw[:size] if size else None


def mono_decompress(codec, stream, out_size=None):
    stream = bytes(stream)
    if out_size is None:
        out_size = int.from_bytes(stream[:4], "little")
    out = ctypes.create_string_buffer(max(out_size, 1))
    size = _lib().hsrle_decompress_mono(codec_id(codec), stream, len(stream), out, out_size)
    return out.raw[:size] if size else None


def mono_tuning(block=0, region=0, lookback=0):
    """Knobs of the monolithic decode (hsrle_mono_tuning): any values give the same output; 0 = the library's choice."""
    _lib().hsrle_mono_tuning(block, region, lookback)


def mono_compress_dev(codec, src, dst=None, workspace=None, return_chunks=False):
    """ONE monolithic reference stream of the CUDA uint8 tensor `src`, written by many lanes (hsrle_compress_mono_dev; the multi-symbol
    codecs of every width and the 8 bit Single codecs: not Greedy, not rle8_single_short).  Returns the stream tensor."""
    import torch

    _check_u8_cuda(src, "src")
    cid = codec_id(codec)
    n = src.numel()
    if dst is None:
        dst = torch.empty(compress_bounds(n) + 64, dtype=torch.uint8, device=src.device)
    need = _lib().hsrle_compress_mono_workspace_size(cid, n)
    if need == 0:
        raise HsrleError(ERR_UNSUPPORTED, "hsrle_compress_mono_dev")
    if workspace is None or workspace.numel() < need:
        workspace = _scratch(need, src.device)
    size, chunks = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _call("hsrle_compress_mono_dev", cid, src, n, dst, dst.numel(), workspace, workspace.numel(), ctypes.byref(size), ctypes.byref(chunks))
    return (dst[: size.value], chunks.value) if return_chunks else dst[: size.value]


def _mono_encode_args(fn, src, dst, workspace, size_out, status=None):
    """Every tensor of an enqueue-only encode checked before the call: a bad one raises HsrleError (ERR_ARGUMENT) here, not a fault on the device later.
    src / dst / workspace: contiguous CUDA uint8 tensors; size_out / status: contiguous CUDA tensors of at least 4 bytes (any dtype)."""
    import torch

    def bad(what, need):
        raise HsrleError(ERR_ARGUMENT, f"{fn}: {what} must be a contiguous CUDA {need}")

    for t, what in ((src, "src"), (dst, "dst"), (workspace, "workspace")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            bad(what, "uint8 tensor")
    for t, what in ((size_out, "size_out"), (status, "status")):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.numel() * t.element_size() >= 4):
            bad(what, "tensor of at least 4 bytes")


def mono_compress_dev_async(codec, src, dst, workspace, size_out=None):
    """hsrle_compress_mono_dev_async (rle8_multi / rle8_packed_multi): enqueue the encode of ONE monolithic reference stream on the current stream; nothing
    synchronises (can be captured in a HIP graph).  dst (>= compress_bounds(n) bytes), workspace (>= hsrle_compress_mono_workspace_size) and size_out
    (uint32[1] or None) are CUDA tensors the caller owns; the stream's size is also in bytes 4 .. 7 of dst once the stream has run."""
    _mono_encode_args("hsrle_compress_mono_dev_async", src, dst, workspace, size_out)
    _call("hsrle_compress_mono_dev_async", codec_id(codec), src, src.numel(), dst, dst.numel(), workspace, workspace.numel(), size_out)


MONO_ENCODE_FAILED = 4


def mono_compress_dev_enqueue(codec, src, dst, workspace, status, size_out=None):
    """hsrle_compress_mono_dev_enqueue: enqueue the encode of ONE monolithic reference stream on the current stream for the 44 codecs whose encoder state at a
    cut the cut fixes (rle8_multi, rle8_packed_multi, plain / Packed of 16 .. 64 bit symbols, Short with no list or a one-symbol list); nothing synchronises (can
    be captured in a HIP graph).  dst (>= compress_bounds(n) bytes) and workspace (>= hsrle_compress_mono_workspace_size) are uint8 CUDA tensors; status and
    size_out (or None) are CUDA tensors of >= 4 bytes, read as one little-endian uint32: MONO_DONE / MONO_ENCODE_FAILED, and the stream's size (0 on failure),
    once the stream has run."""
    if status is None:
        raise HsrleError(ERR_ARGUMENT, "hsrle_compress_mono_dev_enqueue: status is required")
    _mono_encode_args("hsrle_compress_mono_dev_enqueue", src, dst, workspace, size_out, status)
    _call("hsrle_compress_mono_dev_enqueue", codec_id(codec), src, src.numel(), dst, dst.numel(), workspace, workspace.numel(), size_out, status)


def mono_compress_workspace_size(codec, n):
    return int(_lib().hsrle_compress_mono_workspace_size(codec_id(codec), n))


def mono_encode_stats():
    """Of this thread's last monolithic encode with a move-to-front-list codec: (repair rounds, wrong list guesses in round 0, 1, later)."""
    stats = (ctypes.c_uint32 * 4)()
    _lib().hsrle_mono_encode_stats(stats)
    return tuple(int(v) for v in stats)


def mono_decompress_dev(codec, stream_tensor, dst=None, workspace=None, return_stats=False):
    """Decode ONE monolithic reference stream that lives in device memory (uint8 CUDA tensor with >= 64 bytes of slack behind the
    stream's last byte, 128-byte aligned) into device memory.  Returns the output tensor (and (regions, rounds, rewalked, lookback))."""
    import torch

    _check_u8_cuda(stream_tensor, "stream")
    head = stream_tensor[:8].cpu().numpy().tobytes()
    usize, csize = int.from_bytes(head[:4], "little"), int.from_bytes(head[4:8], "little")
    if dst is None:
        dst = torch.empty(max(usize, 1), dtype=torch.uint8, device=stream_tensor.device)
    cid = codec_id(codec)
    need = _lib().hsrle_decompress_mono_workspace_size(cid, usize, csize)
    if workspace is None or workspace.numel() < need:
        workspace = _scratch(max(need, 256), stream_tensor.device)
    n = ctypes.c_uint32(0)
    stats = (ctypes.c_uint32 * 4)()
    _call("hsrle_decompress_mono_dev", cid, stream_tensor, csize, dst, dst.numel(), workspace, workspace.numel(), ctypes.byref(n), stats)
    return (dst[: n.value], tuple(stats)) if return_stats else dst[: n.value]


MONO_DONE, MONO_MALFORMED, MONO_NEEDS_REPAIR = 0, 1, 2


def mono_decompress_dev_async(codec, stream_tensor, header16, dst, workspace, status, stream_size=None):
    """hsrle_decompress_mono_dev_async: enqueue the decode of ONE monolithic reference stream on the current stream, nothing synchronises
    (can be captured in a HIP graph).  header16: the stream's first 16 bytes (host bytes); dst / workspace / status (uint32[1]) are CUDA
    tensors the caller owns.  Returns the uncompressed size; `status` holds MONO_DONE / MONO_MALFORMED / MONO_NEEDS_REPAIR once the stream
    has run."""
    _check_u8_cuda(stream_tensor, "stream")
    header16 = bytes(header16[:16]).ljust(16, b"\0")
    csize = int.from_bytes(header16[4:8], "little") if stream_size is None else int(stream_size)
    n = ctypes.c_uint32(0)
    _call("hsrle_decompress_mono_dev_async", codec_id(codec), stream_tensor, header16, csize, dst, dst.numel(), workspace, workspace.numel(), ctypes.byref(n), status)
    return n.value


def mono_decompress_workspace_size(codec, usize, csize):
    return int(_lib().hsrle_decompress_mono_workspace_size(codec_id(codec), usize, csize))


MONO_INDEX_MISMATCH = 3


def mono_index_size(codec, usize, csize, spacing=0):
    return int(_lib().hsrle_mono_index_size(codec_id(codec), usize, csize, spacing))


def mono_index_build(codec, stream_tensor, spacing=0, index=None, workspace=None, stream_size=None):
    """hsrle_mono_index_build_dev: the persistent entry-point index of ONE monolithic stream in device memory (128-byte aligned, >= 64 bytes
    of slack behind it), one record per `spacing` output bytes (0 = the library's choice).  Synchronous.  Returns (index tensor trimmed to
    its size, MonoIndexInfo); index.cpu() is a file that can be stored beside the stream and loaded again (mono_index_info)."""
    import torch

    _check_u8_cuda(stream_tensor, "stream")
    head = stream_tensor[:8].cpu().numpy().tobytes()
    usize, csize = int.from_bytes(head[:4], "little"), int.from_bytes(head[4:8], "little")
    ssize = csize if stream_size is None else int(stream_size)
    cid = codec_id(codec)
    if index is None:
        need = _lib().hsrle_mono_index_size(cid, usize, csize, spacing)
        if need == 0:
            raise HsrleError(ERR_ARGUMENT, "hsrle_mono_index_size")
        index = torch.empty(need, dtype=torch.uint8, device=stream_tensor.device)
    _check_u8_cuda(index, "index")
    if workspace is None:
        need = _lib().hsrle_mono_index_workspace_size(cid, usize, csize, spacing)
        workspace = _scratch(max(need, 256), stream_tensor.device)
    _check_u8_cuda(workspace, "workspace")
    info = MonoIndexInfo()
    _call("hsrle_mono_index_build_dev", cid, stream_tensor, ssize, spacing, index, index.numel(), workspace, workspace.numel(), ctypes.byref(info))
    return index[: info.indexBytes], info


def mono_index_info(index):
    """Parse and validate an index header (hsrle_mono_index_info_host): host bytes, a CPU tensor or a CUDA tensor (its header is copied)."""
    if hasattr(index, "is_cuda"):
        b = index.cpu().numpy().tobytes() if index.is_cuda else index.numpy().tobytes()
        size = index.numel()
    else:
        b = bytes(index)
        size = len(b)
    info = MonoIndexInfo()
    rc = _lib().hsrle_mono_index_info_host(b, size, ctypes.byref(info))
    if rc != OK:
        raise HsrleError(rc, "hsrle_mono_index_info_host")
    return info


def mono_decompress_range_dev_async(stream_tensor, index, info, offset, length, dst, status, stream=None):
    """hsrle_mono_decompress_range_dev_async: enqueue the decode of output bytes [offset, offset + length) of ONE monolithic stream into
    dst[0, length), from its index (CUDA tensor) and `info` (MonoIndexInfo).  Nothing synchronises (can be captured in a HIP graph).  `status`
    (CUDA uint8 tensor of >= 4 bytes, read as one little-endian uint32) holds MONO_DONE / MONO_MALFORMED / MONO_INDEX_MISMATCH once the stream has run."""
    for t, what in ((stream_tensor, "stream"), (index, "index"), (dst, "dst"), (status, "status")):
        _check_u8_cuda(t, what)
    if status.numel() < 4:
        raise TypeError("status must hold 4 bytes")
    _call("hsrle_mono_decompress_range_dev_async", stream_tensor, index, ctypes.byref(info), offset, length, dst, dst.numel(), status, stream=stream)


def call_dropin(name, data, out_cap):
    """Call one of the rle.h-named exports directly, e.g. call_dropin("rle8_packed_multi_compress", data, cap)."""
    data = bytes(data)
    out = ctypes.create_string_buffer(max(out_cap, 1))
    size = getattr(_lib(), name)(data, len(data), out, out_cap)
    return size, out.raw[:size]


# ----------------------------------------------------------------------------------------------------------------------
# device-resident container path (torch tensors as device memory)


def _stream_ptr(stream=None):
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _ptr(t):
    """What a pointer parameter takes: a tensor's address; None, bytes, byref(...) and integers pass as they are."""
    return ctypes.c_void_p(t.data_ptr()) if hasattr(t, "data_ptr") else t


def _call(name, *args, stream=None, raises=True):
    """One device call by name: tensors become their addresses, sizes and the rest pass as they are, the stream (None: the current one) goes last.
    Raises HsrleError(rc, name) unless the code is OK; raises=False returns it."""
    rc = getattr(_lib(), name)(*[_ptr(a) for a in args], _stream_ptr(stream))
    if raises and rc != OK:
        raise HsrleError(rc, name)
    return rc


def _scratch(n, device):
    """A workspace tensor.  HSRLE_POISON_WORKSPACE=1 (the test suite sets it) fills it with garbage first: the library must not rely on
    a workspace that happens to be zero."""
    import torch

    if os.environ.get("HSRLE_POISON_WORKSPACE") == "1":
        return torch.full((n,), 0xC3, dtype=torch.uint8, device=device)
    return torch.empty(n, dtype=torch.uint8, device=device)


def _check_u8_cuda(t, what):
    import torch

    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
        raise TypeError(f"{what} must be a contiguous CUDA uint8 tensor")


def compress_async(codec, src, dst, block_size=DEFAULT_BLOCK_SIZE, workspace=None, stream=None):
    """Enqueue compression of `src` into the container buffer `dst` (capacity >= container_bound)."""
    _check_u8_cuda(src, "src")
    _check_u8_cuda(dst, "dst")
    if workspace is not None:
        _check_u8_cuda(workspace, "workspace")
    _call("hsrle_compress_dev_async", codec_id(codec), src, src.numel(), dst, dst.numel(), block_size, workspace, workspace.numel() if workspace is not None else 0, stream=stream)


def compress(codec, src, block_size=DEFAULT_BLOCK_SIZE, dst=None):
    """Compress a CUDA uint8 tensor; returns (container tensor trimmed to its size, ContainerInfo)."""
    import torch

    _check_u8_cuda(src, "src")
    if dst is None:
        dst = torch.empty(container_bound(src.numel(), block_size), dtype=torch.uint8, device=src.device)
    total = ctypes.c_uint64(0)
    _call("hsrle_compress_dev", codec_id(codec), src, src.numel(), dst, dst.numel(), block_size, ctypes.byref(total))
    container = dst[: total.value]
    return container, container_info(container)


def container_info(container):
    info = ContainerInfo()
    if hasattr(container, "is_cuda"):
        if container.is_cuda:
            rc = _lib().hsrle_container_info_dev(ctypes.c_void_p(container.data_ptr()), container.numel(), ctypes.byref(info), _stream_ptr())
        else:
            rc = _lib().hsrle_container_info_host(ctypes.c_void_p(container.data_ptr()), container.numel(), ctypes.byref(info))
    else:
        b = bytes(container)
        rc = _lib().hsrle_container_info_host(b, len(b), ctypes.byref(info))
    if rc != OK:
        raise HsrleError(rc, "hsrle_container_info")
    return info


def decompress_async(container, info, dst, status=None, first_block=0, block_count=None, stream=None):
    """Enqueue decompression (of a block range) of a device container into `dst`; `status` is an optional int32/uint32 CUDA tensor."""
    _check_u8_cuda(container, "container")
    _check_u8_cuda(dst, "dst")
    if block_count is None:
        block_count = info.blockCount - first_block
    _call("hsrle_decompress_blocks_dev_async", container, ctypes.byref(info), first_block, block_count, dst, dst.numel(), status, stream=stream)


def decompress_range_dev_async(container, info, offset, length, dst, status, stream=None):
    """hsrle_decompress_range_dev_async: enqueue the decode of output bytes [offset, offset + length) of a device container into dst[0, length)
    (one lane per covering block).  `status` (CUDA uint8 tensor of >= 4 bytes) holds MONO_DONE / MONO_MALFORMED once the stream has run."""
    for t, what in ((container, "container"), (dst, "dst"), (status, "status")):
        _check_u8_cuda(t, what)
    if status.numel() < 4:
        raise TypeError("status must hold 4 bytes")
    _call("hsrle_decompress_range_dev_async", container, ctypes.byref(info), offset, length, dst, dst.numel(), status, stream=stream)


def hash_blocks(container, info, first_block=0, block_count=None):
    """64 bit hash of every block stream (hsrle_hash_blocks_dev_async) as an int64 CUDA tensor (bit pattern of the uint64 values)."""
    import torch

    _check_u8_cuda(container, "container")
    if block_count is None:
        block_count = info.blockCount - first_block
    out = torch.empty(block_count, dtype=torch.int64, device=container.device)
    _call("hsrle_hash_blocks_dev_async", container, ctypes.byref(info), first_block, block_count, out)
    return out


def split_workspace_size(info, block_count=None, sub_block=0):
    return int(_lib().hsrle_decompress_split_workspace_size(ctypes.byref(info), info.blockCount if block_count is None else block_count, sub_block))


def decompress_split_async(container, info, dst, workspace, status=None, sub_block=0, first_block=0, block_count=None, stream=None):
    """Split decode (hsrle_decompress_split_dev_async): one decode lane per `sub_block` output bytes instead of per block."""
    _check_u8_cuda(container, "container")
    _check_u8_cuda(dst, "dst")
    if block_count is None:
        block_count = info.blockCount - first_block
    _call("hsrle_decompress_split_dev_async", container, ctypes.byref(info), first_block, block_count, dst, dst.numel(), status, workspace,
          workspace.numel() if workspace is not None else 0, sub_block, stream=stream)


def decompress_wave_async(container, info, dst, status=None, first_block=0, block_count=None, stream=None):
    """Wave decode (hsrle_decompress_wave_dev_async): one wave per block.  Experiment builds only."""
    if not hasattr(_lib(), "hsrle_decompress_wave_dev_async"):
        raise HsrleError(ERR_UNSUPPORTED, "hsrle_decompress_wave_dev_async (not in the shipped build)")
    _check_u8_cuda(container, "container")
    _check_u8_cuda(dst, "dst")
    if block_count is None:
        block_count = info.blockCount - first_block
    _call("hsrle_decompress_wave_dev_async", container, ctypes.byref(info), first_block, block_count, dst, dst.numel(), status, stream=stream)


def decompress(container, dst=None):
    import torch

    _check_u8_cuda(container, "container")
    info = container_info(container)
    if dst is None:
        dst = torch.empty(info.uncompressedSize, dtype=torch.uint8, device=container.device)
    n = ctypes.c_uint64(0)
    _call("hsrle_decompress_dev", container, container.numel(), dst, dst.numel(), ctypes.byref(n))
    return dst[: n.value]


def synth(kind, symbol_bytes, seed, size, device="cuda", out=None):
    """Deterministic synthetic workload generated on the device; same bytes as the C/python generators."""
    import torch

    if out is None:
        out = torch.empty(size, dtype=torch.uint8, device=device)
    _call("hsrle_synth_dev_async", kind, symbol_bytes, seed, out, size)
    return out


def split_container(container_bytes):
    """Host-side view of a container: (ContainerInfo, [block stream bytes ...])."""
    b = bytes(container_bytes)
    info = container_info(b)
    import struct

    offs = struct.unpack_from(f"<{info.blockCount + 1}Q", b, HEADER_SIZE)
    p0 = info.payload_start
    return info, [b[p0 + offs[i] : p0 + offs[i + 1]] for i in range(info.blockCount)]


# ----------------------------------------------------------------------------------------------------------------------
# rle8m: the reference's own GPU decode path (include/hsrle.h)


def rle8m_info(stream_tensor):
    """Header fields of a device-resident rle8m stream (synchronises)."""
    _check_u8_cuda(stream_tensor, "stream")
    info = Rle8mInfo()
    _call("hsrle_rle8m_info_dev", stream_tensor, stream_tensor.numel(), ctypes.byref(info))
    return info


def rle8m_decompress_async(stream_tensor, info, dst, status=None, stream=None):
    """Enqueue the decode of a device-resident rle8m stream into `dst` (uint8 CUDA tensor); `status` optional int32 tensor."""
    _check_u8_cuda(stream_tensor, "stream")
    _check_u8_cuda(dst, "dst")
    _call("hsrle_rle8m_decompress_dev_async", stream_tensor, ctypes.byref(info), dst, dst.numel(), status, stream=stream)


def rle8m_compress_dropin(sections, data):
    """rle8m_compress(subSections, pIn, inSize, pOut, outSize) of the library (host pointers); returns the stream or None (the reference's 0)."""
    data = bytes(data)
    cap = rle8m_bounds(sections, len(data))
    out = ctypes.create_string_buffer(cap + 64)
    size = _lib().rle8m_compress(sections, data, len(data), out, cap)
    return out.raw[:size] if size else None


def rle8m_compress_async(src, sections, dst, workspace, status=None, stream=None):
    """Enqueue the rle8m encode of the uint8 CUDA tensor `src` into `dst` (capacity >= rle8m_compress_bounds) with `sections` sub-sections."""
    _check_u8_cuda(src, "src")
    _check_u8_cuda(dst, "dst")
    _check_u8_cuda(workspace, "workspace")
    _call("hsrle_rle8m_compress_dev_async", src, src.numel(), sections, dst, dst.numel(), workspace, workspace.numel(), status, stream=stream)


def rle8m_workspace_size(in_size, sections):
    return int(_lib().hsrle_rle8m_compress_workspace_size(in_size, sections))


def rle8m_bounds(sections, in_size):
    return int(_lib().rle8m_compress_bounds(sections, in_size))


def low_entropy_bounds(in_size):
    return int(_lib().rle8_low_entropy_compress_bounds(in_size))


def low_entropy_workspace_size(n):
    """hsrle_low_entropy_workspace_size: bytes of device workspace for the encode of `n` input bytes (0 for n == 0)."""
    return int(_lib().hsrle_low_entropy_workspace_size(n))


def low_entropy_compress_dev(src, variant, dst, workspace, status, stream=None):
    """hsrle_low_entropy_compress_dev_async: enqueue the unsectioned low-entropy encode of the uint8 CUDA tensor `src` into `dst` (capacity >=
    low_entropy_bounds) -- variant: bit 0 the Short form, bit 1 only_max_frequency; `status`: an int32 CUDA tensor, one word.  Nothing is read back: the
    stream's size is its first u32.  Returns the status code (OK, ERR_CAPACITY, ERR_ARGUMENT, ...): returned, not raised."""
    for t, what in ((src, "src"), (dst, "dst"), (workspace, "workspace")):
        _check_u8_cuda(t, what)
    return int(_call("hsrle_low_entropy_compress_dev_async", src, src.numel(), variant, dst, dst.numel(), workspace, workspace.numel(), status, stream=stream, raises=False))


def encode_stats_words(workspace):
    """(prob, pcount), 256 uint32 each: the run statistics a finished low_entropy_compress_dev / rle8m_compress_async left in the first 2 048 bytes of its
    workspace tensor (include/hsrle.h: for tests and measurements)."""
    words = workspace[:2048].cpu().numpy().view("<u4")
    return words[:256].copy(), words[256:].copy()


def low_entropy_decompress_workspace_size(stream_size):
    """hsrle_low_entropy_decompress_workspace_size: bytes of device workspace for the decode of an unsectioned stream of `stream_size` bytes."""
    return int(_lib().hsrle_low_entropy_decompress_workspace_size(stream_size))


def low_entropy_decompress_dev(stream_tensor, dst, workspace, stream=None):
    """hsrle_low_entropy_decompress_dev: decode the device-resident unsectioned low-entropy stream into `dst` (uint8 CUDA tensors; synchronises).
    Returns (status code, uncompressed size): OK, ERR_FORMAT for a stream that is refused, ... -- the code is returned, not raised."""
    for t, what in ((stream_tensor, "stream"), (dst, "dst"), (workspace, "workspace")):
        _check_u8_cuda(t, what)
    size = ctypes.c_uint32(0)
    rc = _call("hsrle_low_entropy_decompress_dev", stream_tensor, stream_tensor.numel(), dst, dst.numel(), workspace, workspace.numel(), ctypes.byref(size), stream=stream, raises=False)
    return int(rc), int(size.value)


def low_entropy_decode_attempts(workspace):
    """Decode attempts of the last low_entropy_decompress_dev on the workspace tensor: 1, or 2 where the one-wave fallback ran (include/hsrle.h)."""
    return int(workspace[8:12].cpu().numpy().view("<u4")[0])


# ----------------------------------------------------------------------------------------------------------------------
# the multi-move-to-front transforms (include/hsrle.h section 5; reference: src/rle.h:420-438)

MMTF128, MMTF256, BITMMTF8, BITMMTF16 = 0, 1, 2, 3
_MMTF_NAMES = ("mmtf128", "mmtf256", "bitmmtf8", "bitmmtf16")


def mmtf_workspace_size(transform, size):
    """hsrle_mmtf_workspace_size: bytes of device workspace of mmtf_dev (0: unknown transform, or a size above 2^32 - 1)."""
    return int(_lib().hsrle_mmtf_workspace_size(transform, size))


def mmtf_tuning(segment_rows=0):
    """hsrle_mmtf_tuning: rows per segment (mmtf128 / mmtf256) / elements per chunk (bitmmtf decodes); 0 = the library's choice.  Process-global,
    for tests; it changes mmtf_workspace_size."""
    _lib().hsrle_mmtf_tuning(segment_rows)


def mmtf_dev(transform, decode, src, dst, ws, stream=None):
    """hsrle_mmtf_dev_async: enqueue one transform of the CUDA uint8 tensor `src` into dst[0, src.numel()) (any byte addresses, not overlapping).
    Nothing synchronises (can be captured in a HIP graph); `ws` holds >= mmtf_workspace_size(transform, src.numel()) bytes, contents irrelevant."""
    for t, what in ((src, "src"), (dst, "dst"), (ws, "ws")):
        _check_u8_cuda(t, what)
    if dst.numel() < src.numel():
        raise TypeError("dst is shorter than src")
    _call("hsrle_mmtf_dev_async", transform, 1 if decode else 0, src, src.numel(), dst, ws, ws.numel(), stream=stream)


def mmtf_bounds(n):
    return int(_lib().mmtf_bounds(n))


def bitmmtf_bounds(n):
    return int(_lib().bitmmtf_bounds(n))


def _mmtf_dropin(name):
    def f(data, out_cap=None):
        """The reference-named host-pointer function: returns (return value, output bytes[:return value])."""
        data = bytes(data)
        return call_dropin(name, data, len(data) if out_cap is None else out_cap)

    f.__name__ = name
    return f


mmtf128_encode, mmtf128_decode = _mmtf_dropin("mmtf128_encode"), _mmtf_dropin("mmtf128_decode")
mmtf256_encode, mmtf256_decode = _mmtf_dropin("mmtf256_encode"), _mmtf_dropin("mmtf256_decode")
bitmmtf8_encode, bitmmtf8_decode = _mmtf_dropin("bitmmtf8_encode"), _mmtf_dropin("bitmmtf8_decode")
bitmmtf16_encode, bitmmtf16_decode = _mmtf_dropin("bitmmtf16_encode"), _mmtf_dropin("bitmmtf16_decode")


# ----------------------------------------------------------------------------------------------------------------------
# rle8_mmtf128: mmtf128 + run-length coding over rank rows + bit packing (include/hsrle.h section 5; reference: src/rle8_mmtf.c)

RLE8_MMTF_DONE, RLE8_MMTF_MALFORMED, RLE8_MMTF_CAPACITY = 0, 1, 2


def rle8_mmtf128_compress_bounds(n):
    return int(_lib().rle8_mmtf128_compress_bounds(n))


def rle8_mmtf256_compress_bounds(n):
    return int(_lib().rle8_mmtf256_compress_bounds(n))


def rle8_mmtf128_compress(data, out_cap=None):
    """The reference-named host-pointer function: returns (return value, stream[:return value]).  out_cap defaults to the reference's bound + 5 (the
    bound itself is 5 bytes short for incompressible input, include/hsrle.h)."""
    data = bytes(data)
    return call_dropin("rle8_mmtf128_compress", data, rle8_mmtf128_compress_bounds(len(data)) + 5 if out_cap is None else out_cap)


def rle8_mmtf128_decompress(stream, out_cap):
    """The reference-named host-pointer function: returns (return value, output[:return value])."""
    return call_dropin("rle8_mmtf128_decompress", bytes(stream), out_cap)


def rle8_mmtf128_workspace_size(decode, size):
    """hsrle_rle8_mmtf128_workspace_size: bytes of device workspace for `size` uncompressed bytes (0: size == 0 or above 2^30)."""
    return int(_lib().hsrle_rle8_mmtf128_workspace_size(1 if decode else 0, size))


def rle8_mmtf_tuning(span_rows=0):
    """hsrle_rle8_mmtf_tuning: rows per wave span of the compress passes (1 .. 64; 0 = 64).  Process-global, for tests."""
    _lib().hsrle_rle8_mmtf_tuning(span_rows)


def rle8_mmtf128_compress_dev(src, dst, out_size, status, ws, stream=None):
    """hsrle_rle8_mmtf128_compress_dev_async: enqueue the compression of the CUDA uint8 tensor `src` into `dst` (>= src.numel() + 8 bytes; + 13 always
    suffice).  out_size / status: CUDA int32 tensors of one element, they receive the stream size and RLE8_MMTF_DONE / RLE8_MMTF_CAPACITY."""
    for t, what in ((src, "src"), (dst, "dst"), (ws, "ws")):
        _check_u8_cuda(t, what)
    _call("hsrle_rle8_mmtf128_compress_dev_async", src, src.numel(), dst, dst.numel(), out_size, status, ws, ws.numel(), stream=stream)


def rle8_mmtf128_decompress_dev(src, dst, status, ws, stream=None):
    """hsrle_rle8_mmtf128_decompress_dev_async: enqueue the decompression of the stream in the CUDA uint8 tensor `src` into `dst`, whose numel() is the
    uncompressed size.  status: CUDA int32 tensor of one element, receives RLE8_MMTF_DONE / RLE8_MMTF_MALFORMED."""
    for t, what in ((src, "src"), (dst, "dst"), (ws, "ws")):
        _check_u8_cuda(t, what)
    _call("hsrle_rle8_mmtf128_decompress_dev_async", src, src.numel(), dst, dst.numel(), status, ws, ws.numel(), stream=stream)


# the entry index of one rle8_mmtf128 stream: a sidecar that lets a wave per stretch follow the header chain (include/hsrle.h section 5)

RLE8_MMTF_INDEX = 3
RLE8_MMTF_INDEX_CODEC = 0xFFFFFFFF
Rle8MmtfIndexInfo = MonoIndexInfo                                        # hsrle_rle8_mmtf128_index_info_t is hsrle_mono_index_info_t


def rle8_mmtf128_index_bound(size, spacing_rows=0):
    """hsrle_rle8_mmtf128_index_bound: an index capacity that always suffices (0: bad spacing, size above 2^30).  spacing_rows 0 = the default."""
    return int(_lib().hsrle_rle8_mmtf128_index_bound(size, spacing_rows))


def rle8_mmtf128_index_info(index):
    """hsrle_rle8_mmtf128_index_info_host on index bytes: the validated header as Rle8MmtfIndexInfo; raises HsrleError(ERR_FORMAT) for a bad one."""
    index = bytes(index)
    info = Rle8MmtfIndexInfo()
    rc = _lib().hsrle_rle8_mmtf128_index_info_host(index, len(index), ctypes.byref(info))
    if rc != OK:
        raise HsrleError(rc, "hsrle_rle8_mmtf128_index_info_host")
    return info


def rle8_mmtf128_compress_indexed_dev(src, dst, out_size, status, ws, index, index_size, spacing_rows=0, stream=None):
    """hsrle_rle8_mmtf128_compress_indexed_dev_async: rle8_mmtf128_compress_dev and the stream's entry index into the CUDA uint8 tensor `index`
    (>= rle8_mmtf128_index_bound bytes).  index_size: CUDA int64 tensor of one element, receives the index size (0: the stream did not fit)."""
    for t, what in ((src, "src"), (dst, "dst"), (ws, "ws"), (index, "index")):
        _check_u8_cuda(t, what)
    _call("hsrle_rle8_mmtf128_compress_indexed_dev_async", src, src.numel(), dst, dst.numel(), out_size, status, ws, ws.numel(), spacing_rows, index, index.numel(), index_size,
          stream=stream)


def rle8_mmtf128_index_build_dev(src, size, index, index_size, status, spacing_rows=0, stream=None):
    """hsrle_rle8_mmtf128_index_build_dev_async: the index of the stream in `src` (of `size` uncompressed bytes), by one serial walk.  status receives
    RLE8_MMTF_DONE or RLE8_MMTF_MALFORMED (then index_size receives 0)."""
    for t, what in ((src, "src"), (index, "index")):
        _check_u8_cuda(t, what)
    _call("hsrle_rle8_mmtf128_index_build_dev_async", src, src.numel(), size, spacing_rows, index, index.numel(), index_size, status, stream=stream)


def rle8_mmtf128_decompress_indexed_dev(src, index, info, dst, status, ws, stream=None):
    """hsrle_rle8_mmtf128_decompress_indexed_dev_async: rle8_mmtf128_decompress_dev with the header chain followed from the entries of `index` (CUDA uint8
    tensor; info: its Rle8MmtfIndexInfo).  status receives RLE8_MMTF_DONE, RLE8_MMTF_MALFORMED or RLE8_MMTF_INDEX (index and stream do not agree)."""
    for t, what in ((src, "src"), (index, "index"), (dst, "dst"), (ws, "ws")):
        _check_u8_cuda(t, what)
    _call("hsrle_rle8_mmtf128_decompress_indexed_dev_async", src, src.numel(), index, ctypes.byref(info), dst, dst.numel(), status, ws, ws.numel(), stream=stream)


def rle8_mmtf128_index_build_host(stream, spacing_rows=0, index_cap=None):
    """hsrle_rle8_mmtf128_index_build_host: (status, index bytes) of a stream in host bytes."""
    stream = bytes(stream)
    cap = rle8_mmtf128_index_bound(int.from_bytes(stream[:4], "little"), spacing_rows) if index_cap is None else index_cap
    out = ctypes.create_string_buffer(max(cap, 1))
    size = ctypes.c_uint64(0)
    rc = _lib().hsrle_rle8_mmtf128_index_build_host(stream, len(stream), spacing_rows, out, cap, ctypes.byref(size))
    return rc, out.raw[: size.value] if rc == OK else b""


def rle8_mmtf128_decompress_indexed_host(stream, index, out_cap):
    """hsrle_rle8_mmtf128_decompress_indexed_host: (status, uncompressed bytes) of a stream and its index in host bytes."""
    stream, index = bytes(stream), bytes(index)
    out = ctypes.create_string_buffer(max(out_cap, 1))
    size = ctypes.c_uint64(0)
    rc = _lib().hsrle_rle8_mmtf128_decompress_indexed_host(stream, len(stream), index, len(index), out, out_cap, ctypes.byref(size))
    return rc, out.raw[: size.value] if rc == OK else b""


# checkpoints of one rle8_mmtf128 stream (the sixteen lists in front of every checkpointRows-th row) and the byte-range decode from index and checkpoints

RLE8_MMTF_CHECKPOINT = 4


class Rle8MmtfCheckpointsInfo(ctypes.Structure):
    """hsrle_rle8_mmtf128_checkpoints_info_t: the header of the checkpoint sidecar of one rle8_mmtf128 stream."""

    _fields_ = [
        ("version", ctypes.c_uint32),
        ("headerBytes", ctypes.c_uint32),
        ("uncompressedSize", ctypes.c_uint32),
        ("streamSize", ctypes.c_uint32),
        ("checkpointRows", ctypes.c_uint32),
        ("checkpointCount", ctypes.c_uint32),
        ("size", ctypes.c_uint64),
    ]


def rle8_mmtf128_checkpoints_bound(size, checkpoint_rows=0):
    """hsrle_rle8_mmtf128_checkpoints_bound: the exact size of the sidecar (0: bad checkpoint_rows, size above 2^30).  checkpoint_rows 0 = the default."""
    return int(_lib().hsrle_rle8_mmtf128_checkpoints_bound(size, checkpoint_rows))


def rle8_mmtf128_checkpoints_info(checkpoints):
    """hsrle_rle8_mmtf128_checkpoints_info_host on sidecar bytes: the validated header as Rle8MmtfCheckpointsInfo; raises HsrleError(ERR_FORMAT) for a bad one."""
    checkpoints = bytes(checkpoints)
    info = Rle8MmtfCheckpointsInfo()
    rc = _lib().hsrle_rle8_mmtf128_checkpoints_info_host(checkpoints, len(checkpoints), ctypes.byref(info))
    if rc != OK:
        raise HsrleError(rc, "hsrle_rle8_mmtf128_checkpoints_info_host")
    return info


def rle8_mmtf128_range_workspace_size(length, spacing_rows=0, checkpoint_rows=0):
    """hsrle_rle8_mmtf128_range_workspace_size: bytes of device workspace of a range decode of `length` bytes (0: bad arguments)."""
    return int(_lib().hsrle_rle8_mmtf128_range_workspace_size(length, spacing_rows, checkpoint_rows))


def rle8_mmtf128_checkpoints_build_dev(src, index, info, checkpoints, size, status, ws, checkpoint_rows=0, stream=None):
    """hsrle_rle8_mmtf128_checkpoints_build_dev_async: the checkpoints of the stream in `src` with its index (info: Rle8MmtfIndexInfo) into the CUDA uint8
    tensor `checkpoints` (>= rle8_mmtf128_checkpoints_bound bytes).  size: CUDA int64 tensor of one element, receives the sidecar's size; status receives
    RLE8_MMTF_DONE, or RLE8_MMTF_MALFORMED / RLE8_MMTF_INDEX (then size receives 0).  ws: rle8_mmtf128_workspace_size(True, n) bytes."""
    for t, what in ((src, "src"), (index, "index"), (checkpoints, "checkpoints"), (ws, "ws")):
        _check_u8_cuda(t, what)
    _call("hsrle_rle8_mmtf128_checkpoints_build_dev_async", src, src.numel(), index, ctypes.byref(info), checkpoint_rows, checkpoints, checkpoints.numel(), size, status, ws,
          ws.numel(), stream=stream)


def rle8_mmtf128_decompress_range_dev(src, index, info, checkpoints, checkpoints_info, offset, length, dst, status, ws, stream=None):
    """hsrle_rle8_mmtf128_decompress_range_dev_async: output bytes [offset, offset + length) of the stream in `src` into dst[0, length), from its index and
    checkpoints (CUDA uint8 tensors; info, checkpoints_info: their headers).  status receives RLE8_MMTF_DONE, _MALFORMED, _INDEX or _CHECKPOINT; dst is
    written behind DONE only.  ws: rle8_mmtf128_range_workspace_size(length, info.spacing, checkpoints_info.checkpointRows) bytes."""
    for t, what in ((src, "src"), (index, "index"), (checkpoints, "checkpoints"), (dst, "dst"), (ws, "ws")):
        _check_u8_cuda(t, what)
    _call("hsrle_rle8_mmtf128_decompress_range_dev_async", src, src.numel(), index, ctypes.byref(info), checkpoints, ctypes.byref(checkpoints_info), offset, length, dst,
          dst.numel(), status, ws, ws.numel(), stream=stream)


def rle8_mmtf128_checkpoints_build_host(stream, index, checkpoint_rows=0, cap=None):
    """hsrle_rle8_mmtf128_checkpoints_build_host: (status, sidecar bytes) of a stream and its index in host bytes."""
    stream, index = bytes(stream), bytes(index)
    cap = rle8_mmtf128_checkpoints_bound(int.from_bytes(stream[:4], "little"), checkpoint_rows) if cap is None else cap
    out = ctypes.create_string_buffer(max(cap, 1))
    size = ctypes.c_uint64(0)
    rc = _lib().hsrle_rle8_mmtf128_checkpoints_build_host(stream, len(stream), index, len(index), checkpoint_rows, out, cap, ctypes.byref(size))
    return rc, out.raw[: size.value] if rc == OK else b""


def rle8_mmtf128_decompress_range_host(stream, index, checkpoints, offset, length, out_cap=None):
    """hsrle_rle8_mmtf128_decompress_range_host: (status, output bytes [offset, offset + length)) of a stream and its two sidecars in host bytes."""
    stream, index, checkpoints = bytes(stream), bytes(index), bytes(checkpoints)
    cap = length if out_cap is None else out_cap
    out = ctypes.create_string_buffer(max(cap, 1))
    rc = _lib().hsrle_rle8_mmtf128_decompress_range_host(stream, len(stream), index, len(index), checkpoints, len(checkpoints), offset, length, out, cap)
    return rc, out.raw[:length] if rc == OK else b""


# ----------------------------------------------------------------------------------------------------------------------
# rle8_sh: run-length coding with a bit stream of capped unary tokens (include/hsrle.h section 5; reference: src/rle_sh.c)

RLE8_SH_DONE, RLE8_SH_MALFORMED, RLE8_SH_CAPACITY = 0, 1, 2


def rle8_sh_bounds(n):
    return int(_lib().rle8_sh_bounds(n))


def rle8_sh_capacity(n):
    """hsrle_rle8_sh_capacity: an output capacity that always suffices for `n` input bytes (include/hsrle.h has the derivation)."""
    return int(_lib().hsrle_rle8_sh_capacity(n))


def rle8_sh_compress(data, out_cap=None):
    """The reference-named host-pointer function: returns (return value, stream[:return value]).  out_cap defaults to rle8_sh_capacity (the
    reference's bound is not one, include/hsrle.h)."""
    data = bytes(data)
    return call_dropin("rle8_sh_compress", data, rle8_sh_capacity(len(data)) if out_cap is None else out_cap)


def rle8_sh_decompress(stream, out_cap):
    """The reference-named host-pointer function: returns (return value, output[:return value])."""
    return call_dropin("rle8_sh_decompress", bytes(stream), out_cap)


def rle8_sh_workspace_size(decode, size):
    """hsrle_rle8_sh_workspace_size: bytes of device workspace for `size` uncompressed bytes (0: size == 0 or above 2^30)."""
    return int(_lib().hsrle_rle8_sh_workspace_size(1 if decode else 0, size))


def rle8_sh_tuning(stretch_symbols=0, walk_window=0, serial_state=0):
    """hsrle_rle8_sh_tuning: symbols per stretch record (1 .. 4096; 0 = 128; a record is never cut inside a word of the bit stream, so below 64
    every word is a record of its own, of up to 64 symbols), bytes per walk window (64 .. 1024; 0 = 1024), serial_state != 0: the decoder's serial
    symbol pass instead of the scan under the guess.  Process-global, for tests."""
    _lib().hsrle_rle8_sh_tuning(stretch_symbols, walk_window, serial_state)


def rle8_sh_decode_words(ws):
    """(fallback ran, stretches whose proof failed) of the last decompress call on the workspace tensor `ws` (include/hsrle.h)."""
    base = (-ws.data_ptr()) % 256
    w = ws[base + 8 : base + 16].cpu().numpy().view("<u4")
    return int(w[0]), int(w[1])


def rle8_sh_compress_dev(src, dst, out_size, status, ws, stream=None):
    """hsrle_rle8_sh_compress_dev_async: enqueue the compression of the CUDA uint8 tensor `src` into `dst` (>= src.numel() + 8 bytes;
    rle8_sh_capacity(src.numel()) always suffices).  out_size / status: CUDA int32 tensors of one element, they receive the stream size and
    RLE8_SH_DONE / RLE8_SH_CAPACITY."""
    for t, what in ((src, "src"), (dst, "dst"), (ws, "ws")):
        _check_u8_cuda(t, what)
    _call("hsrle_rle8_sh_compress_dev_async", src, src.numel(), dst, dst.numel(), out_size, status, ws, ws.numel(), stream=stream)


def rle8_sh_decompress_dev(src, dst, status, ws, stream=None):
    """hsrle_rle8_sh_decompress_dev_async: enqueue the decompression of the stream in the CUDA uint8 tensor `src` into `dst`, whose numel() is the
    uncompressed size.  status: CUDA int32 tensor of one element, receives RLE8_SH_DONE / RLE8_SH_MALFORMED."""
    for t, what in ((src, "src"), (dst, "dst"), (ws, "ws")):
        _check_u8_cuda(t, what)
    _call("hsrle_rle8_sh_decompress_dev_async", src, src.numel(), dst, dst.numel(), status, ws, ws.numel(), stream=stream)


# ----------------------------------------------------------------------------------------------------------------------
# the rle8_sh block container: many independent rle8_sh streams per call (include/hsrle.h section 5)

def rle8_sh_blocks_bound(n, block_size=0):
    """hsrle_rle8_sh_blocks_bound: a container capacity that always suffices (0: bad block size, n == 0, too many blocks).  block_size 0 = 4096."""
    return int(_lib().hsrle_rle8_sh_blocks_bound(n, block_size))


def rle8_sh_blocks_workspace_size(decode, n, block_size=0):
    """hsrle_rle8_sh_blocks_workspace_size: bytes of device workspace; a function of min(blocks, blocks in flight) and the block size."""
    return int(_lib().hsrle_rle8_sh_blocks_workspace_size(1 if decode else 0, n, block_size))


def rle8_sh_blocks_tuning(blocks_in_flight=0):
    """hsrle_rle8_sh_blocks_tuning: blocks per group (0 = the default).  Any value gives the same bytes.  Process-global, for tests."""
    _lib().hsrle_rle8_sh_blocks_tuning(blocks_in_flight)


def rle8_sh_blocks_info(container):
    """Rle8ShBlocksInfo of a container in a CUDA tensor (reads the header, synchronises), a CPU tensor or bytes."""
    info = Rle8ShBlocksInfo()
    if hasattr(container, "is_cuda"):
        if container.is_cuda:
            rc = _lib().hsrle_rle8_sh_blocks_info_dev(ctypes.c_void_p(container.data_ptr()), container.numel(), ctypes.byref(info), _stream_ptr())
        else:
            rc = _lib().hsrle_rle8_sh_blocks_info_host(ctypes.c_void_p(container.data_ptr()), container.numel(), ctypes.byref(info))
    else:
        b = bytes(container)
        rc = _lib().hsrle_rle8_sh_blocks_info_host(b, len(b), ctypes.byref(info))
    if rc != OK:
        raise HsrleError(rc, "hsrle_rle8_sh_blocks_info")
    return info


def rle8_sh_blocks_compress_dev(src, dst, out_size, status, ws, block_size=0, stream=None):
    """hsrle_rle8_sh_compress_blocks_dev_async: enqueue the compression of the CUDA uint8 tensor `src` into the container buffer `dst`
    (rle8_sh_blocks_bound always suffices).  out_size: CUDA int64 tensor of one element, receives the container's size (0: it did not fit);
    status: CUDA int32 tensor of one element, receives RLE8_SH_DONE / RLE8_SH_CAPACITY."""
    for t, what in ((src, "src"), (dst, "dst"), (ws, "ws")):
        _check_u8_cuda(t, what)
    _call("hsrle_rle8_sh_compress_blocks_dev_async", src, src.numel(), block_size, dst, dst.numel(), out_size, status, ws, ws.numel(), stream=stream)


def rle8_sh_blocks_decompress_dev(container, info, dst, status, ws, first_block=0, block_count=None, stream=None):
    """hsrle_rle8_sh_decompress_blocks_dev_async: enqueue the decompression of blocks [first_block, first_block + block_count) of the container in
    the CUDA uint8 tensor `container` into `dst` (>= info.uncompressedSize bytes; block i lands at i * blockSize).  status: CUDA int32 tensor of one
    element, receives RLE8_SH_DONE / RLE8_SH_MALFORMED."""
    for t, what in ((container, "container"), (dst, "dst"), (ws, "ws")):
        _check_u8_cuda(t, what)
    count = info.blockCount - first_block if block_count is None else block_count
    _call("hsrle_rle8_sh_decompress_blocks_dev_async", container, ctypes.byref(info), first_block, count, dst, dst.numel(), status, ws, ws.numel(), stream=stream)


def rle8_sh_blocks_compress_host(data, block_size=0, out_cap=None):
    """hsrle_rle8_sh_compress_blocks_host: (status, container bytes) of host bytes.  out_cap defaults to rle8_sh_blocks_bound."""
    data = bytes(data)
    cap = rle8_sh_blocks_bound(len(data), block_size) if out_cap is None else out_cap
    out = ctypes.create_string_buffer(max(cap, 1))
    total = ctypes.c_uint64(0)
    rc = _lib().hsrle_rle8_sh_compress_blocks_host(data, len(data), block_size, out, cap, ctypes.byref(total))
    return rc, out.raw[: total.value] if rc == OK else b""


def rle8_sh_blocks_decompress_host(container, out_cap):
    """hsrle_rle8_sh_decompress_blocks_host: (status, uncompressed bytes) of a container in host bytes."""
    container = bytes(container)
    out = ctypes.create_string_buffer(max(out_cap, 1))
    size = ctypes.c_uint64(0)
    rc = _lib().hsrle_rle8_sh_decompress_blocks_host(container, len(container), out, out_cap, ctypes.byref(size))
    return rc, out.raw[: size.value] if rc == OK else b""


# ----------------------------------------------------------------------------------------------------------------------
# the rle8_mmtf128 block container: many independent rle8_mmtf128 streams per call, identity lists at every block start (include/hsrle.h section 5)

def rle8_mmtf128_blocks_bound(n, block_size=0):
    """hsrle_rle8_mmtf128_blocks_bound: a container capacity that always suffices (0: bad block size, n == 0, too many blocks).  block_size 0 = 4096."""
    return int(_lib().hsrle_rle8_mmtf128_blocks_bound(n, block_size))


def rle8_mmtf128_blocks_workspace_size(decode, n, block_size=0):
    """hsrle_rle8_mmtf128_blocks_workspace_size: bytes of device workspace; a function of min(blocks, blocks in flight) and the block size."""
    return int(_lib().hsrle_rle8_mmtf128_blocks_workspace_size(1 if decode else 0, n, block_size))


def rle8_mmtf128_blocks_tuning(blocks_in_flight=0):
    """hsrle_rle8_mmtf128_blocks_tuning: blocks per group (0 = the default).  Any value gives the same bytes.  Process-global, for tests."""
    _lib().hsrle_rle8_mmtf128_blocks_tuning(blocks_in_flight)


def rle8_mmtf128_blocks_info(container):
    """Rle8ShBlocksInfo (both block containers share it) of an rle8_mmtf128 block container in a CUDA tensor (reads the header, synchronises), a CPU tensor or bytes."""
    info = Rle8ShBlocksInfo()
    if hasattr(container, "is_cuda"):
        if container.is_cuda:
            rc = _lib().hsrle_rle8_mmtf128_blocks_info_dev(ctypes.c_void_p(container.data_ptr()), container.numel(), ctypes.byref(info), _stream_ptr())
        else:
            rc = _lib().hsrle_rle8_mmtf128_blocks_info_host(ctypes.c_void_p(container.data_ptr()), container.numel(), ctypes.byref(info))
    else:
        b = bytes(container)
        rc = _lib().hsrle_rle8_mmtf128_blocks_info_host(b, len(b), ctypes.byref(info))
    if rc != OK:
        raise HsrleError(rc, "hsrle_rle8_mmtf128_blocks_info")
    return info


def rle8_mmtf128_blocks_compress_dev(src, dst, out_size, status, ws, block_size=0, stream=None):
    """hsrle_rle8_mmtf128_compress_blocks_dev_async: enqueue the compression of the CUDA uint8 tensor `src` into the container buffer `dst`
    (rle8_mmtf128_blocks_bound always suffices).  out_size: CUDA int64 tensor of one element, receives the container's size (0: it did not fit);
    status: CUDA int32 tensor of one element, receives RLE8_MMTF_DONE / RLE8_MMTF_CAPACITY."""
    for t, what in ((src, "src"), (dst, "dst"), (ws, "ws")):
        _check_u8_cuda(t, what)
    _call("hsrle_rle8_mmtf128_compress_blocks_dev_async", src, src.numel(), block_size, dst, dst.numel(), out_size, status, ws, ws.numel(), stream=stream)


def rle8_mmtf128_blocks_decompress_dev(container, info, dst, status, ws, first_block=0, block_count=None, stream=None):
    """hsrle_rle8_mmtf128_decompress_blocks_dev_async: enqueue the decompression of blocks [first_block, first_block + block_count) of the container in
    the CUDA uint8 tensor `container` into `dst` (>= info.uncompressedSize bytes; block i lands at i * blockSize).  status: CUDA int32 tensor of one
    element, receives RLE8_MMTF_DONE / RLE8_MMTF_MALFORMED."""
    for t, what in ((container, "container"), (dst, "dst"), (ws, "ws")):
        _check_u8_cuda(t, what)
    count = info.blockCount - first_block if block_count is None else block_count
    _call("hsrle_rle8_mmtf128_decompress_blocks_dev_async", container, ctypes.byref(info), first_block, count, dst, dst.numel(), status, ws, ws.numel(), stream=stream)


def rle8_mmtf128_blocks_compress_host(data, block_size=0, out_cap=None):
    """hsrle_rle8_mmtf128_compress_blocks_host: (status, container bytes) of host bytes.  out_cap defaults to rle8_mmtf128_blocks_bound."""
    data = bytes(data)
    cap = rle8_mmtf128_blocks_bound(len(data), block_size) if out_cap is None else out_cap
    out = ctypes.create_string_buffer(max(cap, 1))
    total = ctypes.c_uint64(0)
    rc = _lib().hsrle_rle8_mmtf128_compress_blocks_host(data, len(data), block_size, out, cap, ctypes.byref(total))
    return rc, out.raw[: total.value] if rc == OK else b""


def rle8_mmtf128_blocks_decompress_host(container, out_cap):
    """hsrle_rle8_mmtf128_decompress_blocks_host: (status, uncompressed bytes) of a container in host bytes."""
    container = bytes(container)
    out = ctypes.create_string_buffer(max(out_cap, 1))
    size = ctypes.c_uint64(0)
    rc = _lib().hsrle_rle8_mmtf128_decompress_blocks_host(container, len(container), out, out_cap, ctypes.byref(size))
    return rc, out.raw[: size.value] if rc == OK else b""
