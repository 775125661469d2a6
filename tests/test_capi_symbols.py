"""The C-ABI library loads (no GPU needed) and exports every symbol include/hsrle.h declares; no compute calls here."""
import ctypes
import os
import re

import pytest

import hsrle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "hypersonic-rle-kit_amd", "libhsrle_hip.so")
HEADER = os.path.join(REPO, "include", "hsrle.h")


def prototypes(experiments=False):
    """{symbol: (return type, [parameter types])} of every function include/hsrle.h declares, its macros expanded.  A type is its base name without
    const, with a * per pointer level (an array parameter is a pointer).  experiments: the declarations inside #ifdef HSRLE_EXPERIMENTS instead (not part
    of the shipped library)."""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    guarded = re.compile(r"#ifdef HSRLE_EXPERIMENTS(.*?)#endif", re.S)
    text = "".join(guarded.findall(text)) if experiments else guarded.sub("", text)
    text = text.replace("\\\n", " ")
    macros = {m.group(1): (m.group(2), m.group(3)) for m in re.finditer(r"^#define\s+(\w+)\((\w+)\)\s+(.*)$", text, flags=re.M)}   # the drop-in declarators: one parameter each
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    call = re.compile(r"\b(%s)\((\w+)\)" % "|".join(macros or ["(?!)"]))
    while call.search(text):
        text = call.sub(lambda m: re.sub(r"\s*##\s*", "", re.sub(r"\b%s\b" % macros[m.group(1)][0], m.group(2), macros[m.group(1)][1])), text)
    text = re.sub(r"typedef\s+(?:struct|enum)[^{;]*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)

    def ctype(decl, named):
        stars = decl.count("*") + decl.count("[")
        words = re.sub(r"\[[^\]]*\]|\*|\bconst\b", " ", decl).split()
        return " ".join(words[:-1] if named and len(words) > 1 else words) + "*" * stars

    out = {}
    for ret, name, params in re.findall(r"([\w\s\*]+?)\b(\w+)\s*\(([^()]*)\)\s*;", text):
        params = [q.strip() for q in params.split(",") if q.strip() not in ("", "void")]
        out[name] = (ctype(ret, False), [ctype(q, True) for q in params])
    return out


def declared_symbols():
    return sorted(prototypes())


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess

        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(REPO, "hypersonic-rle-kit_amd")])
    return hsrle.declare(ctypes.CDLL(LIB))


def test_all_declared_symbols_are_exported(lib):
    syms = declared_symbols()
    assert len(syms) >= 2 + 100 + 88 + 15 + 15  # helpers + 50 extreme + 44 Short drop-in pairs + 15 Greedy encoders + hsrle_* API
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, f"not exported: {missing}"


def test_reference_names_present(lib):
    """Exactly the names of the reference's rle.h for the hot path (src/rle.h:100-394)."""
    for s in ("rle_compress_bounds", "rle_decompress_additional_size", "rle8_multi_compress", "rle8_single_compress", "rle8_decompress",
              "rle8_packed_multi_compress", "rle8_packed_single_compress", "rle8_packed_decompress", "rle64_3symlut_byte_compress",
              "rle64_3symlut_byte_decompress", "rle24_sym_packed_compress", "rle128_byte_packed_decompress",
              "rle8_multi_short_compress", "rle8_1symlut_short_decompress", "rle16_sym_short_compress", "rle48_7symlut_byte_short_decompress",
              "rle8m_opencl_init", "rle8m_opencl_destroy", "rle8m_opencl_decompress", "rle8m_decompress", "rle8m_compress", "rle8m_compress_bounds"):
        assert hasattr(lib, s)


def test_pure_host_helpers(lib):
    """Helpers that need no device."""
    assert lib.rle_compress_bounds(1000) == 1193
    assert lib.rle_compress_bounds((1 << 30) + 1) == 0
    assert lib.rle_decompress_additional_size() == 128
    for i in range(110):
        name = lib.hsrle_codec_name(i)
        assert lib.hsrle_codec_from_name(name) == i
    assert lib.hsrle_codec_from_name(b"rle8_packed_multi") == 1 and lib.hsrle_codec_from_name(b"rle64_3symlut_byte") == 44
    assert lib.hsrle_codec_from_name(b"nope") == -1
    assert lib.hsrle_container_bound(1 << 20, 4096) > (1 << 20)
    assert lib.hsrle_container_bound(1 << 20, 4000) == 0  # block size must be a multiple of 128


def test_encode_path_selection(lib):
    """hsrle_encode_path (no device): which encoder a container takes.  Big containers: one lane per block; small ones of 1 .. 4 KiB blocks: the
    run list encoders for the multi-symbol 8 bit codecs, the 2 .. 8 byte codecs and their Short family, the split encode for the rest that
    can be cut (Single, 128 bit and Greedy only with a workspace sized for the codec); other block sizes: split encode or ring."""
    cid = lambda n: lib.hsrle_codec_from_name(n.encode())
    RING, SPLIT, RUN_LIST, PP = 0, 1, 2, 3
    frame = 88473600
    # rounds 5 / 6: the position-parallel encoders take every container of <= 4 KiB blocks of their 93 codecs (all 50 extreme codecs among them), whatever its size
    for name in ("rle8_multi", "rle8_packed_multi", "rle16_sym", "rle16_byte_packed", "rle24_sym_packed", "rle32_byte_packed", "rle48_3symlut_sym", "rle64_3symlut_byte", "rle24_3symlut_byte",
                 "rle16_sym_short", "rle16_1symlut_sym_short", "rle24_byte_short", "rle48_1symlut_byte_short", "rle64_sym_short",
                 "rle8_multi_short", "rle8_1symlut_short", "rle48_3symlut_sym_short", "rle64_3symlut_byte_short",
                 "rle8_3symlut", "rle8_7symlut", "rle16_3symlut_sym", "rle16_3symlut_byte", "rle16_7symlut_byte", "rle24_7symlut_byte", "rle64_7symlut_sym",
                 "rle16_3symlut_sym_short", "rle32_3symlut_byte_short", "rle64_7symlut_byte_short", "rle24_7symlut_sym_short",
                 "rle8_single", "rle8_packed_single", "rle8_single_short", "rle128_sym", "rle128_sym_packed", "rle128_byte", "rle128_byte_packed"):
        assert cid(name) >= 0
        for size, block in ((frame, 4096), (frame, 1024), (frame, 512), (8 << 30, 4096), (4096, 128)):
            assert lib.hsrle_encode_path(cid(name), size, block) == PP, (name, size, block)
        # round 6: blocks above 4 KiB walked in 4 KiB windows (csrc/hsrle_encode8pw.hip.h, hsrle_encodeSpw.hip.h, hsrle_encodeLpw.hip.h): the two 8 bit multi-symbol codecs, the 54
        # codecs of hsrle_encodeSp.hip.h and the 30 of hsrle_encodeLp.hip.h -- plain / Packed with blocks of any size, the LUT / Short forms below 1 MiB per block (their field
        # widths and penalties go by value).  Not windowed: the 8 bit Single codecs and the 128 bit codecs
        windowed_any = name in ("rle8_multi", "rle8_packed_multi", "rle16_sym", "rle16_byte_packed", "rle24_sym_packed", "rle32_byte_packed")
        windowed_list = name not in ("rle8_single", "rle8_packed_single", "rle8_single_short", "rle128_sym", "rle128_sym_packed", "rle128_byte", "rle128_byte_packed") and not windowed_any
        if windowed_any or windowed_list:
            for size, block in ((frame, 8192), (8 << 30, 8192), (8 << 30, 65536), (1 << 20, 1 << 19), (frame, 4224)):
                assert lib.hsrle_encode_path(cid(name), size, block) == PP, (name, size, block)
            assert (lib.hsrle_encode_path(cid(name), 8 << 30, 1 << 20) == PP) == windowed_any, name
            continue
        assert lib.hsrle_encode_path(cid(name), frame, 8192) == SPLIT, name         # a wave holds 4 KiB: larger blocks by chunks
        assert lib.hsrle_encode_path(cid(name), 8 << 30, 8192) == RING, name
    for name in ("rle8_3symlut_short", "rle8_7symlut_short"):      # (the two Short codecs with a list that are not position-parallel: every pair of equal bytes would be a candidate)
        assert cid(name) >= 0
        assert lib.hsrle_encode_path(cid(name), frame, 4096) == RUN_LIST, name
        assert lib.hsrle_encode_path(cid(name), frame, 1024) == RUN_LIST, name
        assert lib.hsrle_encode_path(cid(name), 8 << 30, 4096) == RING, name        # 2 097 152 blocks
        assert lib.hsrle_encode_path(cid(name), frame, 8192) == SPLIT, name         # run list: blocks of 1 .. 4 KiB only
        assert lib.hsrle_encode_path(cid(name), frame, 512) == RING, name
    for name in ("rle16_1symlut_byte_short_greedy", "rle16_3symlut_byte_short_greedy"):
        assert lib.hsrle_encode_path(cid(name), frame, 4096) == RING, name          # (split only with a workspace sized for the codec -- the host cannot know)
    for name in ("rle16_1symlut_byte_short_greedy", "rle64_1symlut_byte_short_greedy", "rle8_single_short"):
        assert lib.hsrle_encode_path(cid(name), frame, 8192) == SPLIT, name         # round 4: their chunk encoders take the blocks of a container too
    general = lib.hsrle_compress_workspace_size(frame, 4096)
    assert lib.hsrle_compress_workspace_size_codec(cid("rle8_packed_multi"), frame, 4096) == general
    assert lib.hsrle_compress_workspace_size_codec(cid("rle8_single"), frame, 4096) == general          # round 6: position-parallel, no split regions
    assert lib.hsrle_compress_workspace_size_codec(cid("rle8_single_short"), frame, 4096) == general
    assert lib.hsrle_compress_workspace_size_codec(cid("rle16_1symlut_byte_short_greedy"), frame, 4096) > 2 * frame > general
    assert lib.hsrle_compress_workspace_size_codec(cid("rle32_1symlut_byte_short_greedy"), frame, 4096) > 2 * frame
    for name in ("rle16_3symlut_byte_short_greedy", "rle64_7symlut_byte_short_greedy"):     # lists of 3 / 7 symbols decide the greedy scan's runs: one lane per block
        assert lib.hsrle_encode_path(cid(name), frame, 8192) == RING and lib.hsrle_compress_workspace_size_codec(cid(name), frame, 4096) == general
    assert lib.hsrle_compress_workspace_size_codec(cid("rle128_sym"), 8 << 30, 4096) == lib.hsrle_compress_workspace_size(8 << 30, 4096)
    # round 6: blocks above 4 KiB of a windowed codec never take the split encode: no split regions in the codec's own workspace size (the general size keeps them)
    for name in ("rle8_packed_multi", "rle32_byte", "rle64_3symlut_byte", "rle16_7symlut_sym"):
        assert lib.hsrle_compress_workspace_size_codec(cid(name), frame, 8192) < 1.2 * frame < lib.hsrle_compress_workspace_size(frame, 8192), name
    assert lib.hsrle_compress_workspace_size_codec(cid("rle128_sym"), frame, 8192) == lib.hsrle_compress_workspace_size(frame, 8192)      # (not windowed: split encode)
    assert lib.hsrle_encode_path(cid("rle8_single_short"), frame, 4096) == PP and lib.hsrle_compress_workspace_size_codec(cid("rle8_single_short"), frame, 4096) == general   # round 6
    assert lib.hsrle_encode_path(-1, frame, 4096) == -1 and lib.hsrle_encode_path(0, frame, 1000) == -1 and lib.hsrle_encode_path(0, 0, 4096) == -1


def test_decode_ring_rule(lib):
    """hsrle_decode_ring (no device): the stream ring of the plain block decode.  The rule, stated here independently of csrc/hsrle_codecs.h: the
    64-byte ring iff (payloadSize + 32) * 1000 < uncompressedSize * T with T = 250 for 1 / 2 byte symbols and 215 for 3 / 4 byte symbols; 6, 8 and
    16 byte symbols take 128 at any ratio.  Every codec id, the last payload size on the small side and the first on the other, at a size whose
    products need 64 bits too."""
    from hsrle_testlib import CODECS

    assert not lib.hsrle_experiments_enabled() or not os.environ.get("HSRLE_DEC_RING"), "an experiments build with a forced ring does not follow the rule"
    for cid, c in enumerate(CODECS):
        T = 250 if c.S <= 2 else 215 if c.S <= 4 else 0
        for U in (4096, 1000000, 786432 + 2053, (8 << 30) + 12345, 1 << 44):
            if T == 0:
                for payload in (0, 1, U // 8, U // 4, U, 2 * U):
                    assert lib.hsrle_decode_ring(cid, U, payload) == 128, (c.key, U, payload)
                continue
            edge = -(-U * T // 1000)                 # smallest payload + 32 that is NOT below the threshold: ceil(U * T / 1000)
            assert (edge - 1) * 1000 < U * T <= edge * 1000
            assert lib.hsrle_decode_ring(cid, U, edge - 32 - 1) == 64, (c.key, U)
            assert lib.hsrle_decode_ring(cid, U, edge - 32) == 128, (c.key, U)
            assert lib.hsrle_decode_ring(cid, U, 0) == 64 and lib.hsrle_decode_ring(cid, U, U) == 128, (c.key, U)
    assert lib.hsrle_decode_ring(-1, 4096, 10) == -1 and lib.hsrle_decode_ring(110, 4096, 10) == -1
    assert lib.hsrle_decode_ring(0, 0, 0) == 128      # (no such container; nothing is below a threshold of 0 bytes)


def test_codec_table_matches_tests_table(lib):
    from hsrle_testlib import CODECS

    assert [lib.hsrle_codec_name(i).decode() for i in range(110)] == [c.key for c in CODECS]
