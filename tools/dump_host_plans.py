#!/usr/bin/env python3
"""What the device-free planning entry points of libhsrle_hip.so return, for every codec over a fixed grid: the host side's behaviour as data.

  python tools/dump_host_plans.py [out.json]        (HSRLE_LIB=<path> picks another build of the library)
  python tools/dump_host_plans.py --stream [out.json]   the stream codecs' plans alone (tests/golden/host_plans_stream.json)

tests/golden/host_plans.json is this tool's output for the build the codec traits table (csrc/hsrle_codecs.h) replaced;
its "codec_free" rows (the low-entropy and rle8m workspaces, which take no codec id) were written from the build before
csrc/hsrle_capi.hip was cut into its csrc/hsrle_capi_*.h parts and the three scan-level layouts became one.
tests/test_host_plans.py asserts that the current build reproduces it value for value.  None of the calls below touches a device.
hsrle_mono_tuning() is never called: the plans are those of the defaults.
"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("HSRLE_LIB", os.path.join(REPO, "hypersonic-rle-kit_amd", "libhsrle_hip.so"))

SIZES32 = [4096, (1 << 20) + 128, 88473600, 1 << 30]
SIZES64 = SIZES32 + [8 << 30]
BLOCKS = [128, 1024, 4096, 4224, 8192, 65536, 1 << 20]
SPACINGS = [0, 512, 4096]
SECTIONS = [1, 7, 4096, 262144]


def compressed_sizes(U):
    return [U // 8, U]


def load(path=LIB):
    sys.path.insert(0, os.path.join(REPO, "hypersonic-rle-kit_amd", "python"))
    import hsrle                                                         # (the signature table; importing it needs neither torch nor a device)

    return hsrle.declare(ctypes.CDLL(path))


def dump(L):
    """{entry point: {"vectors": the distinct value lists in grid order, "codec": {codec name: which of them}}} -- most codecs share a plan"""
    names = []
    while True:
        nm = L.hsrle_codec_name(len(names))
        if nm is None:
            break
        names.append(nm.decode())
    calls = {
        "hsrle_encode_path": lambda c: [L.hsrle_encode_path(c, U, B) for U in SIZES64 for B in BLOCKS],
        "hsrle_compress_workspace_size_codec": lambda c: [L.hsrle_compress_workspace_size_codec(c, U, B) for U in SIZES64 for B in BLOCKS],
        "hsrle_compress_mono_workspace_size": lambda c: [L.hsrle_compress_mono_workspace_size(c, U) for U in SIZES32],
        "hsrle_decompress_mono_workspace_size": lambda c: [L.hsrle_decompress_mono_workspace_size(c, U, C) for U in SIZES32 for C in compressed_sizes(U)],
        "hsrle_mono_index_size": lambda c: [L.hsrle_mono_index_size(c, U, C, sp) for U in SIZES32 for C in compressed_sizes(U) for sp in SPACINGS],
        "hsrle_mono_index_workspace_size": lambda c: [L.hsrle_mono_index_workspace_size(c, U, C, sp) for U in SIZES32 for C in compressed_sizes(U) for sp in SPACINGS],
    }
    out = {}
    for fn, call in calls.items():
        vectors, which = [], {}
        for c, nm in enumerate(names):
            v = call(c)
            if v not in vectors:
                vectors.append(v)
            which[nm] = vectors.index(v)
        out[fn] = {"vectors": vectors, "codec": which}
    return {"grid": {"sizes32": SIZES32, "sizes64": SIZES64, "blocks": BLOCKS, "compressed": ["U/8", "U"], "spacings": SPACINGS}, "results": out, "codec_free": dump_codec_free(L)}


def dump_codec_free(L):
    """the plans that take no codec id, over SIZES32 (rle8m: x SECTIONS, sizes outermost)"""
    return {
        "sections": SECTIONS,
        "hsrle_low_entropy_workspace_size": [L.hsrle_low_entropy_workspace_size(U) for U in SIZES32],
        "hsrle_low_entropy_decompress_workspace_size": [L.hsrle_low_entropy_decompress_workspace_size(U) for U in SIZES32],
        "hsrle_rle8m_compress_workspace_size": [L.hsrle_rle8m_compress_workspace_size(U, n) for U in SIZES32 for n in SECTIONS],
    }


STREAM_SIZES = [1, 15, 16, 4096, (1 << 20) + 128, 1 << 30, (1 << 30) + 1]
STREAM_BLOCKS = [0, 128, 4096, 65536, 1 << 20, 192]   # 0: the default; 192: no multiple of 128, refused
TRANSFORMS = ["mmtf128", "mmtf256", "bitmmtf8", "bitmmtf16"]


def dump_stream(L):
    """the plans of the stream codecs (rle8_sh, rle8_mmtf128, the mmtf transforms, the rle8_sh block container) over STREAM_SIZES: rows with a direction
    are {"compress": ..., "decompress": ...}, the transforms' one row each, the container's rows sizes outermost x STREAM_BLOCKS.  Tunings at their defaults."""
    both = lambda call: {"compress": call(0), "decompress": call(1)}   # noqa: E731
    return {
        "sizes": STREAM_SIZES,
        "blocks": STREAM_BLOCKS,
        "hsrle_rle8_sh_workspace_size": both(lambda d: [L.hsrle_rle8_sh_workspace_size(d, U) for U in STREAM_SIZES]),
        "hsrle_rle8_sh_capacity": [L.hsrle_rle8_sh_capacity(U) for U in STREAM_SIZES],
        "rle8_sh_bounds": [L.rle8_sh_bounds(U) for U in STREAM_SIZES],
        "hsrle_rle8_mmtf128_workspace_size": both(lambda d: [L.hsrle_rle8_mmtf128_workspace_size(d, U) for U in STREAM_SIZES]),
        "rle8_mmtf128_compress_bounds": [L.rle8_mmtf128_compress_bounds(U) for U in STREAM_SIZES],
        "hsrle_mmtf_workspace_size": {nm: [L.hsrle_mmtf_workspace_size(t, U) for U in STREAM_SIZES] for t, nm in enumerate(TRANSFORMS)},
        "hsrle_rle8_sh_blocks_bound": [L.hsrle_rle8_sh_blocks_bound(U, B) for U in STREAM_SIZES for B in STREAM_BLOCKS],
        "hsrle_rle8_sh_blocks_workspace_size": both(lambda d: [L.hsrle_rle8_sh_blocks_workspace_size(d, U, B) for U in STREAM_SIZES for B in STREAM_BLOCKS]),
    }


def expand(results):
    """{entry point: {codec name: values}}"""
    return {fn: {nm: r["vectors"][k] for nm, k in r["codec"].items()} for fn, r in results.items()}


if __name__ == "__main__":
    if sys.argv[1:2] == ["--stream"]:
        text = "{\n%s\n}" % ",\n".join(' "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in dump_stream(load()).items())
        with (open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout) as f:
            f.write(text + "\n")
        sys.exit(0)
    d = dump(load())
    # one line per entry point and part: short enough to read, few enough lines to review
    rows = ['  "%s": {"vectors": %s,\n    "codec": %s}' % (fn, json.dumps(r["vectors"], separators=(",", ":")), json.dumps(r["codec"], separators=(",", ":"))) for fn, r in d["results"].items()]
    free = ",\n".join('  "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in d["codec_free"].items())
    text = '{"grid": %s,\n "results": {\n%s\n },\n "codec_free": {\n%s\n }}' % (json.dumps(d["grid"]), ",\n".join(rows), free)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    else:
        print(text)
