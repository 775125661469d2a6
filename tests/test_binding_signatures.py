"""The binding's signature table (hsrle.SIGNATURES, applied by hsrle.declare) against the prototypes of include/hsrle.h, symbol for symbol.  A function with
no declaration takes ctypes' default of int and truncates a 64 bit size without a word, and a wrong one is no better: every declared function must have an
entry whose restype and argtypes are the prototype's types under one fixed mapping, and the table must name nothing the library does not export.  No GPU."""
import ctypes
import os

import pytest

import hsrle
from test_capi_symbols import LIB, prototypes

INTEGERS = {"int": ctypes.c_int, "uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "bool": ctypes.c_bool}
INFO_STRUCTS = {"hsrle_container_info_t": hsrle.ContainerInfo, "hsrle_rle8_sh_blocks_info_t": hsrle.Rle8ShBlocksInfo, "hsrle_mono_index_info_t": hsrle.MonoIndexInfo,
                "hsrle_rle8m_info_t": hsrle.Rle8mInfo}
OTHER_STRUCTS = ("rle8_low_entropy_compress_info_t", "rle8_low_entropy_decompress_info_t")   # the reference's own tables (src/rle.h): the package has no class for them


def allowed(ctype):
    """the ctypes types a C type may be bound as"""
    if ctype == "void":
        return [None]
    if not ctype.endswith("*"):
        return [INTEGERS[ctype]]                                         # scalars map to themselves
    base = ctype.rstrip("*")
    if ctype.count("*") == 2:
        assert base == "void", ctype
        return [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    if base == "char":
        return [ctypes.c_char_p]
    if base in INFO_STRUCTS:
        return [ctypes.POINTER(INFO_STRUCTS[base])]
    if base == "void" or base in OTHER_STRUCTS:
        return [ctypes.c_void_p]
    return [ctypes.c_void_p, ctypes.POINTER(INTEGERS[base])]             # a pointer to an integer: untyped, or typed where a caller passes byref of one


def test_the_parser_reads_the_header():
    P = prototypes()
    assert P["hsrle_codec_name"] == ("char*", ["int"]) and P["rle_decompress_additional_size"] == ("uint32_t", [])
    assert P["hsrle_mono_encode_stats"] == ("void", ["uint32_t*"])       # an array parameter
    assert P["rle48_7symlut_byte_short_decompress"] == ("uint32_t", ["uint8_t*", "uint32_t", "uint8_t*", "uint32_t"])      # a macro inside a macro
    assert P["rle16_3symlut_byte_short_compress_greedy"] == P["mmtf128_encode"] == P["rle8_sh_compress"] == P["rle48_7symlut_byte_short_decompress"]
    assert P["hsrle_rccl_comm_create"] == ("int", ["void*", "int", "int", "void**"])
    assert P["hsrle_rle8_sh_decompress_blocks_dev_async"] == ("int", ["void*", "hsrle_rle8_sh_blocks_info_t*", "uint32_t", "uint32_t", "void*", "uint64_t", "uint32_t*", "void*",
                                                                      "uint64_t", "void*"])
    assert sum(sig == ("uint32_t", ["uint8_t*", "uint32_t", "uint8_t*", "uint32_t"]) for sig in P.values()) >= 205   # the reference-named drop-in functions
    assert len(P) >= 327 and not any(name.endswith("_t") for name in P)


def check(table, protos):
    assert sorted(table) == sorted(protos), f"without an entry: {sorted(set(protos) - set(table))}; entries the header does not declare: {sorted(set(table) - set(protos))}"
    wrong = []
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        if restype not in allowed(ret):
            wrong.append(f"{name}: returns {ret}, bound as {restype}")
        if len(argtypes) != len(params):
            wrong.append(f"{name}: {len(params)} parameters, {len(argtypes)} argtypes")
            continue
        wrong += [f"{name}: parameter {i} is {c}, bound as {t}" for i, (c, t) in enumerate(zip(params, argtypes)) if t not in allowed(c)]
    assert not wrong, "\n".join(wrong)


def test_every_prototype_has_its_entry():
    check(hsrle.SIGNATURES, prototypes())


def test_experiment_prototypes_have_their_guarded_entries():
    check(hsrle.EXPERIMENT_SIGNATURES, prototypes(experiments=True))


def test_the_table_names_only_what_the_library_exports():
    if not os.path.exists(LIB):
        pytest.fail("libhsrle_hip.so is not built")
    L = ctypes.CDLL(LIB)
    assert [name for name in hsrle.SIGNATURES if not hasattr(L, name)] == []
    hsrle.declare(L)
    for name, (restype, argtypes) in hsrle.SIGNATURES.items():
        f = getattr(L, name)
        assert f.restype == restype and list(f.argtypes) == list(argtypes), name
    for name in hsrle.EXPERIMENT_SIGNATURES:                             # declared where the build has them, left alone where it has not
        assert hasattr(L, name) == bool(L.hsrle_experiments_enabled()), name
