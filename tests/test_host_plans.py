"""The host side plans what it planned before the codec traits table (csrc/hsrle_codecs.h) replaced the codec-id arithmetic: tools/dump_host_plans.py over
the current build against tests/golden/host_plans.json, which the same tool wrote from the build of the commit before -- encode path, container / monolithic
encode and decode workspaces, index size and index workspace, for all 110 codecs over a grid of sizes, block sizes, compressed sizes and record spacings.
The "codec_free" rows do the same for the workspaces that take no codec id (low-entropy encode and decode, rle8m encode over four section counts); they
were written from the build before the three hand-rolled scan-level layouts became one.  No device is touched."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
GOLDEN = os.path.join(REPO, "tests", "golden", "host_plans.json")


def test_host_plans_are_the_recorded_ones():
    import dump_host_plans

    if not os.path.exists(dump_host_plans.LIB):
        import subprocess

        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(REPO, "hypersonic-rle-kit_amd")])
    with open(GOLDEN) as f:
        want = json.load(f)
    got = dump_host_plans.dump(dump_host_plans.load())
    assert got["grid"] == want["grid"]
    got, want = dump_host_plans.expand(got["results"]), dump_host_plans.expand(want["results"])
    assert sorted(got) == sorted(want)
    for fn, per_codec in want.items():
        assert list(got[fn]) == list(per_codec), f"{fn}: codec names or their order differ"
        assert len(per_codec) == 110
        for name, values in per_codec.items():
            assert got[fn][name] == values, f"{fn}({name})"


def test_codec_free_plans_are_the_recorded_ones():
    import dump_host_plans

    with open(GOLDEN) as f:
        want = json.load(f)["codec_free"]
    got = dump_host_plans.dump_codec_free(dump_host_plans.load())
    assert sorted(got) == sorted(want)
    assert len(want["hsrle_rle8m_compress_workspace_size"]) == len(dump_host_plans.SIZES32) * len(want["sections"])
    for fn, values in want.items():
        assert got[fn] == values, fn


def test_stream_codec_plans_are_the_recorded_ones():
    """tests/golden/host_plans_stream.json: the stream codecs' workspace sizes, capacities and bounds (rle8_sh, rle8_mmtf128, the four mmtf transforms, the
    rle8_sh block container), written by `dump_host_plans.py --stream` from the build before their plans took the shared round-up of csrc/hsrle_capi_host.h"""
    import dump_host_plans

    with open(os.path.join(REPO, "tests", "golden", "host_plans_stream.json")) as f:
        want = json.load(f)
    got = dump_host_plans.dump_stream(dump_host_plans.load())
    assert list(got) == list(want)
    assert want["sizes"] == [1, 15, 16, 4096, (1 << 20) + 128, 1 << 30, (1 << 30) + 1] and want["blocks"] == [0, 128, 4096, 65536, 1 << 20, 192]
    assert len(want["hsrle_rle8_sh_blocks_bound"]) == len(want["sizes"]) * len(want["blocks"])
    for fn, values in want.items():
        assert got[fn] == values, fn
