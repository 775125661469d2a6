"""csrc/hsrle_codecs.h against an independent table: a small host program (plain g++, no HIP) prints every row of kCodecs and what the accessors derive from
it; name, family, symbol bytes and alignment must be those of hsrle_testlib.CODECS (built from the reference's naming scheme, not from the header), the list
length the one the name states, codec_id() the inverse of the table, and the stream header 9 bytes for the four 8 bit plain / Packed codecs and 8 elsewhere.
The decode rule (decode_variant: which k_decode_blocks instantiation a launch takes) is printed for every row and case and compared with the rule written out here.
So is the encode rule (encode_choice: which encoder takes a container and which split regions its workspace gets): every row with what its row of the launch table has
(written out here per family), over the sizes and block sizes of tests/golden/host_plans.json x the three kinds of workspace x noSplit; for the workspace every caller
has, the printed path must be the hsrle_encode_path that file recorded from the library.  The decode entry points' argument checks are printed in their order."""
import os
import re
import subprocess

import pytest

import hsrle_testlib as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "hypersonic-rle-kit_amd", "csrc", "hsrle_codecs.h")

PROGRAM = r"""
#include "%s"
#include <stdio.h>
using namespace hsrle;
int main()
{
  for (int c = 0; c < kCodecCount; c++)
  {
    const CodecInfo &i = kCodecs[c];
    printf("%%d %%s %%d %%d %%d %%d %%d %%d %%u %%u %%d %%u\n", c, i.name, (int)i.fam, (int)i.S, (int)i.aligned, (int)i.greedy, list_len(i), state_slots(i), header_size(i), cut_long(i),
           codec_id(i.fam, i.S, i.aligned, i.greedy), small_ring_per_mille(i));
    for (int k = 0; k < 8; k++)   // bit 2: output window, bit 1: entry records, bit 0: the small-ring predicate said yes
    {
      const DecodeVariant v = decode_variant(i, (k & 4) != 0, (k & 2) != 0, (k & 1) != 0);
      printf("variant %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", c, k, (int)v.fam, (int)v.sgl, (int)v.ent, (int)v.win, v.ring, (int)v.list8, (int)v.pe);
    }
  }
  // the encode rule: every row with what its row of the launch table has (written out by the test), over the grid of tests/golden/host_plans.json
  const EncodeCaps caps[kCodecCount] = { %s };
  const uint64_t sizes[] = { %s };
  const uint32_t blocks[] = { %s };
  for (int c = 0; c < kCodecCount; c++)
    for (unsigned u = 0; u < sizeof sizes / sizeof *sizes; u++)
      for (unsigned b = 0; b < sizeof blocks / sizeof *blocks; b++)
        for (int have = 0; have < 3; have++)
          for (int noSplit = 0; noSplit < 2; noSplit++)
          {
            const EncodeChoice e = encode_choice(kCodecs[c], caps[c], sizes[u], blocks[b], block_count(sizes[u], blocks[b]), (SplitRegions)have, noSplit != 0);
            printf("encode %%d %%u %%u %%d %%d %%d %%d %%d %%d\n", c, u, b, have, noSplit, (int)e.path, (int)e.ppw, (int)e.runList, (int)e.regions);
          }
  // the decode entry points' argument checks, in their order: a null pointer, a bad info, a bad range, a short output
  hsrle_container_info_t good = { 1, 1, 7 * 1024 + 100, 1024, 8, 100, 0 }, badCodec = good, badBlock = good, badCount = good;
  badCodec.codec = kCodecCount; badBlock.blockSize = 1000; badCount.blockCount = 9;
  const char out = 0;
  printf("prologue %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", decode_info_check(nullptr, &badCodec, &out), decode_info_check(&out, nullptr, &out), decode_info_check(&out, &badCodec, nullptr),
         decode_info_check(&out, &badCodec, &out), decode_info_check(&out, &badBlock, &out), decode_info_check(&out, &badCount, &out), decode_info_check(&out, &good, &out),
         decode_range_check(good, 7, 2, 0), decode_range_check(good, 0xFFFFFFFFu, 2, 0), decode_range_check(good, 0, 8, good.uncompressedSize - 1), decode_range_check(good, 8, 0, good.uncompressedSize));
  return 0;
}
"""

# hsrle_testlib family -> (Family value in the header, greedy flag): the Greedy encoders are rows of SHORT1 / 3 / 7 with the flag set
FAMILY = {T.PLAIN: (0, 0), T.PACKED: (1, 0), T.LUT3: (2, 0), T.LUT7: (3, 0), T.SINGLE: (4, 0), T.PACKED_SINGLE: (5, 0), T.SHORT0: (6, 0), T.SHORT1: (7, 0),
          T.SHORT3: (8, 0), T.SHORT7: (9, 0), T.GREEDY1: (7, 1), T.GREEDY3: (8, 1), T.GREEDY7: (9, 1), T.SINGLE_SHORT: (10, 0)}


# ---- what a codec's row of the launch table has (csrc/inst_*.hip), per family: the encode rule's second input ----
LUT3_, LUT7_, SHORT0_, SHORT1_, SHORT3_, SHORT7_, SHORT_SINGLE_ = 2, 3, 6, 7, 8, 9, 10
PPW_NONE, PPW_8, PPW_L, PPW_S = 0, 1, 2, 3


def _caps(c):
    """(pp, windowed launcher, menc, enc) of hsrle_testlib codec c: 93 codecs have a position-parallel encoder -- all but Greedy and the 8 bit Short codecs with a list of
    3 / 7 symbols --, 86 of them a windowed one -- not the 8 bit Single codecs, not the 128 bit ones: the 8 bit pair its own, the general LUT kernel's codecs L (7 symbols;
    3 symbols with symbols of 1 / 2 bytes, Short: of 2 .. 4 bytes), the others S; every codec has the ring encoder and a chunk encoder."""
    fam, greedy = FAMILY[c.family]
    single = fam in (4, 5, SHORT_SINGLE_)
    pp = not greedy and not (c.S == 1 and fam in (SHORT3_, SHORT7_))
    if not pp or single or c.S == 16:
        ppw = PPW_NONE
    elif c.S == 1 and fam in (0, 1):
        ppw = PPW_8
    elif fam in (LUT7_, SHORT7_) or (fam == LUT3_ and c.S <= 2) or (fam == SHORT3_ and c.S <= 4):
        ppw = PPW_L
    else:
        ppw = PPW_S
    return int(pp), ppw, 1, 1


def _plans_grid():
    import sys

    sys.path.insert(0, os.path.join(REPO, "tools"))
    import dump_host_plans

    return dump_host_plans


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    d = tmp_path_factory.mktemp("codec_traits")
    src, exe = d / "traits.cpp", d / "traits"
    grid = _plans_grid()
    caps = ", ".join("{ %s, (PpwKind)%d, %s, %s }" % tuple(str(bool(v)).lower() if k != 1 else v for k, v in enumerate(_caps(c))) for c in T.CODECS)
    src.write_text(PROGRAM % (HEADER, caps, ", ".join("%dull" % u for u in grid.SIZES64), ", ".join("%du" % b for b in grid.BLOCKS)))
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", str(src), "-o", str(exe)])
    return subprocess.check_output([str(exe)], text=True).splitlines()


@pytest.fixture(scope="module")
def rows(output):
    keys = ("id", "name", "fam", "S", "aligned", "greedy", "K", "slots", "header", "cut", "found", "ring")
    table = [{k: (v if k == "name" else int(v)) for k, v in zip(keys, line.split())} for line in output if line[0].isdigit()]
    for r in table:
        r["variants"] = {}
    vkeys = ("fam", "sgl", "ent", "win", "ring", "list8", "pe")
    for line in output:
        if line.startswith("variant"):
            c, k, *v = [int(x) for x in line.split()[1:]]
            table[c]["variants"][k] = dict(zip(vkeys, v))
    return table


def test_one_row_per_codec_in_id_order(rows):
    assert len(rows) == len(T.CODECS) == 110
    assert [r["id"] for r in rows] == list(range(110))


def test_rows_are_the_test_tables(rows):
    for r, c in zip(rows, T.CODECS):
        fam, greedy = FAMILY[c.family]
        assert (r["name"], r["fam"], r["S"], r["aligned"], r["greedy"]) == (c.key, fam, c.S, c.aligned, greedy), c.key


def test_list_length_is_what_the_name_says(rows):
    for r in rows:
        m = re.search(r"(\d)symlut", r["name"])
        assert r["K"] == (int(m.group(1)) if m else 0), r["name"]
        assert r["slots"] == (1 if "packed" in r["name"] else r["K"]), r["name"]   # a Packed decoder keeps the last symbol, a list codec its list


def test_codec_id_finds_every_row(rows):
    assert [r["found"] for r in rows] == list(range(110))


def test_header_size(rows):
    nine = {"rle8_multi", "rle8_packed_multi", "rle8_single", "rle8_packed_single"}
    for r in rows:
        assert r["header"] == (9 if r["name"] in nine else 8), r["name"]


def test_every_codec_has_a_cut_length(rows):
    assert all(r["cut"] > r["S"] for r in rows)


def test_small_ring_threshold_goes_by_the_symbol_width(rows):
    """The decoder's 64-byte stream ring: below a quarter for 1 / 2 byte symbols, below 0.215 for 3 / 4 byte symbols, never for wider ones."""
    for r in rows:
        assert r["ring"] == (250 if r["S"] <= 2 else 215 if r["S"] <= 4 else 0), r["name"]


# ---- the decode rule: every row x (output window, entry records, small-ring predicate) ----
PLAIN_, PACKED_, SINGLE_, PACKED_SINGLE_ = 0, 1, 4, 5


def _expected_variant(r, window, entries, small):
    """The table of DESIGN.md 4.1 (first case that applies), from the row's name, family number and symbol bytes alone."""
    fam = {SINGLE_: PLAIN_, PACKED_SINGLE_: PACKED_}.get(r["fam"], r["fam"])      # Single ids decode with the multi kernels; a Greedy row's family IS its Short decoder
    sgl = 0 if r["id"] in (0, 1) else 1
    list8 = 1 if r["S"] == 1 and fam in (PLAIN_, PACKED_) else 0
    if window:
        ent, win, ring = 1, 1, 128
    elif r["S"] == 1:
        ent, win, ring = 1, 0, 64 if (not entries and small) else 128
    elif entries:
        sgl, ent, win, ring = 1, 1, 0, 128
    else:
        sgl, ent, win, ring = 1, 0, 0, 64 if (small and r["S"] <= 4) else 128
    return {"fam": fam, "sgl": sgl, "ent": ent, "win": win, "ring": ring, "list8": list8, "pe": 0}


def _cases(rows):
    for r in rows:
        assert sorted(r["variants"]) == list(range(8)), r["name"]
        for k, v in r["variants"].items():
            yield r, bool(k & 4), bool(k & 2), bool(k & 1), v


def test_decode_rule_is_the_table(rows):
    n = 0
    for r, window, entries, small, v in _cases(rows):
        assert v == _expected_variant(r, window, entries, small), (r["name"], window, entries, small)
        n += 1
    assert n == 110 * 8                                                  # the four cases of the table, each with the ring predicate false and true


def test_decode_rule_properties(rows):
    no_sgl, ring64, no_ent = set(), set(), set()
    for r, window, entries, small, v in _cases(rows):
        if not v["sgl"]:
            no_sgl.add(r["id"])
        if v["ring"] == 64:
            ring64.add(r["id"])
            assert not window and not entries and small, r["name"]      # only a plain container the predicate chose
        else:
            assert v["ring"] == 128
        if not v["ent"]:
            no_ent.add(r["id"])
            assert r["S"] >= 2 and not window and not entries, r["name"]
        elif r["S"] >= 2:
            assert window or entries, r["name"]                          # ENT = 0 EXACTLY for the plain containers of 2 byte symbols and wider
        if v["win"]:
            assert window and v["ent"] and v["ring"] == 128, r["name"]
        else:
            assert not window
        assert not v["pe"]                                               # (an experiment build's knob; none is set here)
        assert v["list8"] == (1 if r["S"] == 1 and v["fam"] in (PLAIN_, PACKED_) else 0), r["name"]
    assert no_sgl == {0, 1}                                              # rle8_multi, rle8_packed_multi -- in their WIN kernel too
    assert all(not v["sgl"] for r, *_, v in _cases(rows) if r["id"] in (0, 1))
    assert ring64 == {r["id"] for r in rows if r["S"] <= 4}
    assert no_ent == {r["id"] for r in rows if r["S"] >= 2}


def test_decode_family_of_single_and_greedy_ids(rows):
    by_name = {r["name"]: r for r in rows}
    for r in rows:
        fams = {v["fam"] for v in r["variants"].values()}
        assert len(fams) == 1, r["name"]                                 # one grammar per codec, whatever the launch
        fam = fams.pop()
        if r["name"] == "rle8_single":
            assert fam == PLAIN_
        elif r["name"] == "rle8_packed_single":
            assert fam == PACKED_
        elif r["greedy"]:
            short = by_name[r["name"][: -len("_greedy")]]
            assert not short["greedy"] and fam == short["fam"] and r["variants"] == short["variants"], r["name"]
        else:
            assert fam == r["fam"], r["name"]


# ---- the encode rule: every row x the host_plans grid x the workspace's split regions x noSplit ----
ENC_PP, ENC_PPW, ENC_SPLIT, ENC_RING_CHUNKS, ENC_RING = 2, 3, 4, 5, 6     # (0: no ring encoder in the row, 1: the experiment builds' wave encoder)
SPLIT_NONE, SPLIT_LARGE, SPLIT_ALL = 0, 1, 2
PATH_RING, PATH_SPLIT, PATH_RUN_LIST, PATH_PP = 0, 1, 2, 3                # include/hsrle.h: HSRLE_PATH_*


def _expected_encode(r, caps, U, B, have, no_split):
    """The table of DESIGN.md 4.2 (first case that applies; the shipped build: no knob set, so a container is one piece), from the row's family, symbol bytes and
    Greedy flag and from what its row of the launch table has.  Returns (path, windowed launcher, run list, regions of the path's workspace)."""
    pp, ppw, menc, enc = caps
    n_blocks = (U + B - 1) // B
    single, plain_packed = r["fam"] in (SINGLE_, PACKED_SINGLE_, SHORT_SINGLE_), r["fam"] in (PLAIN_, PACKED_) and r["S"] <= 8
    greedy_one = r["greedy"] and r["fam"] == SHORT1_
    few_blocks = n_blocks < 131072
    if pp and B <= 4096:
        return ENC_PP, PPW_NONE, 0, SPLIT_LARGE
    if ppw and B > 4096 and (plain_packed or B <= (1 << 20) - 128) and n_blocks * ((B + 4095) // 4096) <= 0xFFFFFFF0:
        return ENC_PPW, ppw, 0, SPLIT_NONE
    run_list = not single and r["S"] != 16 and not r["greedy"] and not pp and 1024 <= B <= 4096 and few_blocks
    if B <= 4096:      # the small-block regions: only the codecs without a run list encoder use them, and the second attempt after a struck container does without
        regions = have == SPLIT_ALL and not no_split and (single or r["S"] == 16 or greedy_one)
    else:
        regions = have != SPLIT_NONE
    if (regions and menc and not run_list and few_blocks and 1024 <= B <= 1 << 20 and B % 512 == 0 and (not r["greedy"] or greedy_one) and not (single and B > 32768)):
        return ENC_SPLIT, PPW_NONE, 0, SPLIT_ALL if B <= 4096 else SPLIT_LARGE
    return ENC_RING, PPW_NONE, int(run_list and U >= 1024), SPLIT_LARGE


def _encode_lines(output):
    for line in output:
        if line.startswith("encode"):
            c, u, b, have, no_split, *answer = [int(x) for x in line.split()[1:]]
            yield c, u, b, have, no_split, tuple(answer)


def test_encode_rule_is_the_table(output, rows):
    grid = _plans_grid()
    n, seen = 0, set()
    for c, u, b, have, no_split, answer in _encode_lines(output):
        want = _expected_encode(rows[c], _caps(T.CODECS[c]), grid.SIZES64[u], grid.BLOCKS[b], have, no_split)
        assert answer == want, (rows[c]["name"], grid.SIZES64[u], grid.BLOCKS[b], have, no_split)
        seen.add((answer[0], answer[1]))
        n += 1
    assert n == 110 * len(grid.SIZES64) * len(grid.BLOCKS) * 3 * 2
    # every outcome of the shipped build occurs on the grid (the chunked ring and the wave encoder need a knob)
    assert seen == {(ENC_PP, PPW_NONE), (ENC_PPW, PPW_8), (ENC_PPW, PPW_L), (ENC_PPW, PPW_S), (ENC_SPLIT, PPW_NONE), (ENC_RING, PPW_NONE)}


def test_encode_rule_answers_hsrle_encode_path_for_the_generic_workspace(output, rows):
    """The printed path for a workspace without the small-block regions is what tests/golden/host_plans.json recorded from the library for the same cell: the
    capabilities written in _caps are the launch table's."""
    import json

    grid = _plans_grid()
    with open(os.path.join(REPO, "tests", "golden", "host_plans.json")) as f:
        recorded = grid.expand(json.load(f)["results"])["hsrle_encode_path"]
    to_public = {ENC_PP: PATH_PP, ENC_PPW: PATH_PP, ENC_SPLIT: PATH_SPLIT}
    n = 0
    for c, u, b, have, no_split, (path, ppw, run_list, regions) in _encode_lines(output):
        if have == SPLIT_LARGE:
            want = recorded[rows[c]["name"]][u * len(grid.BLOCKS) + b]
            assert to_public.get(path, PATH_RUN_LIST if run_list else PATH_RING) == want, (rows[c]["name"], grid.SIZES64[u], grid.BLOCKS[b], no_split)
            n += 1
    assert n == 110 * len(grid.SIZES64) * len(grid.BLOCKS) * 2


def test_encode_rule_properties(output, rows):
    upgraded = set()
    by_cell = {}
    for c, u, b, have, no_split, answer in _encode_lines(output):
        by_cell[(c, u, b, have, no_split)] = answer
    for (c, u, b, have, no_split), (path, ppw, run_list, regions) in by_cell.items():
        assert (ppw != PPW_NONE) == (path == ENC_PPW) and (not run_list or path == ENC_RING)
        assert (regions == SPLIT_NONE) == (path == ENC_PPW)                 # a windowed codec's workspace is planned without the split regions, every other with them
        if regions == SPLIT_ALL:
            assert path == ENC_SPLIT and have == SPLIT_ALL and not no_split
            upgraded.add(rows[c]["name"])
        # the regions change the answer only between the split encode and the ring / run list encoders; noSplit only where the small-block regions would have been used
        base = by_cell[(c, u, b, SPLIT_NONE, no_split)]
        assert (path, ppw, run_list) == base[:3] or (path == ENC_SPLIT and base[0] == ENC_RING)
        if no_split:
            other = by_cell[(c, u, b, have, 0)]
            assert (path, ppw, run_list, regions) == other or (other[3] == SPLIT_ALL and path == ENC_RING)
    assert upgraded == {r["name"] for r in rows if r["greedy"] and r["fam"] == SHORT1_}     # the five Greedy codecs with a one-symbol list


def test_decode_prologue_checks_in_order(output):
    """csrc/hsrle_codecs.h decode_info_check / decode_range_check: a null pointer (1 = HSRLE_ERR_ARGUMENT) beats a bad info (3 = HSRLE_ERR_FORMAT), which beats a block
    range outside the container (1), which beats a short output (2 = HSRLE_ERR_CAPACITY); an empty range is in order."""
    (line,) = [l for l in output if l.startswith("prologue")]
    assert [int(x) for x in line.split()[1:]] == [1, 1, 1, 3, 3, 3, 0, 1, 1, 2, 0]
