"""The lazy run fill of the 8 bit packet loop of k_decode_blocks (hsrle_codecs.h: dec8_lazy_fill) on streams whose runs are PLACED against its 16-byte chunks and
128-byte steps (tests/decode_run_fill_fixtures.py): runs that start at chunk offset 0, 1 and 15 and are 15 ... 113 bytes long, runs that end exactly on a chunk and on
a step boundary, a run over three steps and more, two runs back to back, literal - run - literal inside one chunk, a run up to the block's very end -- all of them in
every wave, beside neighbours that finish each step in one packet.  A lazy kernel stores only the first chunk of what a run fills and leaves the chunks inside the run
to the flush; the bytes must not depend on who writes them.

Every codec id of one-byte symbols whose kernel has uncapped rounds; blocks of 384 and 4 096 bytes; 65 blocks; last blocks of 1, 127 and B - 1 bytes; a sparse mixture
(the 64-byte ring, nearly every chunk inside a run) and a dense one (the 128-byte ring); the plain decode of the whole container and of block ranges (a full wave, a
partial wave), the decode from entry records (one lane per 128 bytes: lanes start in the middle of runs) and the windowed decode, whose kernel keeps the stores.  The
expected bytes are the writers' intended output; the CPU part below proves that the streams parse to it and counts, from the packet lists, that every named form is in
every container.  The malformed containers must end with exactly the status the parent of the change reported for them (tests/golden/decode_run_fill_status.json,
recorded once from the parent's build with record_verdicts below), with the guards around the output untouched and the healthy neighbours decoded.  With A/B builds of
the library present (variants/libhsrle_dec8lazy0.so, ...1.so: tools/build_variant_tu.sh inst_w8 dec8lazy1 -DHSRLE_DEC8_LAZY=1) the same checks run on each of them in a
child process.  The helpers are those of test_gpu_decode_variants.py."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import decode_run_fill_fixtures as R
import stream_grammar as G
from hsrle_testlib import REPO

GOLDEN = os.path.join(REPO, "tests", "golden", "decode_run_fill_status.json")
VARIANTS = ("plain", "windowed", "entries")
CASES = [(c, m) for c in R.CODECS8 for m in R.MIXTURES]
SHAPES = [(B, n) for B in R.BLOCK_SIZES for n in R.LAST_LENGTHS(B)]
ids = lambda v: getattr(v, "key", v)


@pytest.mark.parametrize("codec, mixture", CASES, ids=ids)
def test_fixtures_hold_every_form(codec, mixture):
    """CPU: every stream parses to its intended bytes, every named run placement occurs in every container, and the mixtures lie on their side of the ring rule."""
    g = G.grammar(codec)
    for B, last_len in SHAPES:
        fix, blks = R.container(codec, mixture, B, last_len)
        what = f"{codec.key} {mixture} B {B} last {last_len}"
        assert len(blks) == R.BLOCKS and fix.U == (R.BLOCKS - 1) * B + last_len
        have = collections.Counter()
        for i, blk in enumerate(blks):
            blen = last_len if i == R.BLOCKS - 1 else B
            assert G.parse(g, blk.stream)[0] == blk.out and len(blk.out) == blen, f"{what}: block {i}"
            have.update(R.properties(blk, blen))
        missing = [k for k in R.SPECIAL + ("I",) if not have[k]]
        assert not missing, f"{what}: no block has {missing}"
        assert have["I"] >= 10, f"{what}: too few neighbours that finish a step in one packet"
        assert (have["Ct"] >= 1) == (last_len >= 127), f"{what}: the last block's run must reach its last byte"
        lazy = sum(R.lazy_chunks(b) for b in blks) / (fix.U / R.CHUNK)
        if mixture == "sparse":
            assert fix.ratio <= 0.18 and lazy >= 0.8, f"{what}: ratio {fix.ratio:.3f}, {lazy:.2f} of the chunks inside a run"
        else:
            assert fix.ratio >= 0.40 and lazy >= 0.1, f"{what}: ratio {fix.ratio:.3f}, {lazy:.2f} of the chunks inside a run"
    for what in R.MALFORMED:
        for B in R.BLOCK_SIZES:
            s = R.malformed_container(codec, mixture, B, what).streams[R.VICTIM]
            with pytest.raises(AssertionError):
                G.parse(g, s)


# ----------------------------------------------------------------------------------------------------------------------------------------------------------
# GPU


def _helpers():
    import test_gpu_decode_variants as V

    return V


def _workspace(hs, info):
    import torch

    return torch.full((max(hs.split_workspace_size(info, None, R.SUB_BLOCK), 16),), 0xC3, dtype=torch.uint8, device="cuda")


def check_placed(hs, codec, mixture):
    import torch

    V = _helpers()
    for B, last_len in SHAPES:
        fix, _ = R.container(codec, mixture, B, last_len)
        what = f"{codec.key} {mixture} B {B} last {last_len}"
        ring = V._named_ring(hs, fix, what)
        assert ring == (64 if mixture == "sparse" else 128)
        container, info = V._upload(hs, fix)
        assert info.blockCount == R.BLOCKS
        arena, status = V.Arena(fix.U), V._status()
        for first, count in ((0, R.BLOCKS), (0, 64), (63, 2), (64, 1)):
            arena.reset()
            hs.decompress_async(container, info, arena.view, status, first_block=first, block_count=count)
            V._check_blocks(fix, arena, status, first, count, f"{what} ring {ring} blocks [{first}, +{count})")
        arena.reset()
        hs.decompress_split_async(container, info, arena.view, _workspace(hs, info), status, sub_block=R.SUB_BLOCK)
        V._check_blocks(fix, arena, status, 0, R.BLOCKS, f"{what} from entry records at every {R.SUB_BLOCK} bytes")
        runs = []
        for off, n in R.window_ranges(fix):
            a, st = V.Arena(n), torch.zeros(4, dtype=torch.uint8, device="cuda")
            hs.decompress_range_dev_async(container, info, off, n, a.view, st)
            runs.append((off, n, a, st))
        torch.cuda.synchronize()
        for off, n, a, st in runs:
            w = f"{what} window [{off}, +{n})"
            assert int.from_bytes(st.cpu().numpy().tobytes(), "little") == hs.MONO_DONE == 0, f"{w}: status"
            out, guards = a.host()
            assert np.array_equal(out, fix.data[off : off + n]), f"{w}: differs from the intended bytes"
            assert guards, f"{w}: bytes outside the output were written"


def verdict(hs, fix, variant):
    """(status word, guards untouched, the output bytes and the offset of their first byte) of one decode variant of a container with a malformed block"""
    import torch

    V = _helpers()
    container, info = V._upload(hs, fix)
    if variant == "windowed":
        off, n = R.victim_window(fix)
        arena, st = V.Arena(n), torch.zeros(4, dtype=torch.uint8, device="cuda")
        hs.decompress_range_dev_async(container, info, off, n, arena.view, st)
        torch.cuda.synchronize()
        word = int.from_bytes(st.cpu().numpy().tobytes(), "little")
    else:
        off, arena, st = 0, V.Arena(fix.U), V._status()
        if variant == "plain":
            hs.decompress_async(container, info, arena.view, st)
        else:
            hs.decompress_split_async(container, info, arena.view, _workspace(hs, info), st, sub_block=R.SUB_BLOCK)
        torch.cuda.synchronize()
        word = int(st.item()) & 0xFFFFFFFF
    out, guards = arena.host()
    return word, guards, out, off


def record_verdicts(hs):
    """{golden key: status word} of every malformed container: run ONCE with the parent's library to write the golden file.  One word per codec, malformed kind
    and variant: both mixtures and both block sizes must give the same."""
    words = {}
    for c in R.CODECS8:
        for m in R.MIXTURES:
            for B in R.BLOCK_SIZES:
                for what in R.MALFORMED:
                    for v in VARIANTS:
                        word = verdict(hs, R.malformed_container(c, m, B, what), v)[0]
                        assert words.setdefault(R.golden_key(c, what, v), word) == word, (c.key, m, B, what, v)
    return words


def check_malformed(hs, codec, mixture):
    golden = json.load(open(GOLDEN))
    for B in R.BLOCK_SIZES:
        for what in R.MALFORMED:
            fix = R.malformed_container(codec, mixture, B, what)
            for variant in VARIANTS:
                w = f"{codec.key} {mixture} B {B}, block {R.VICTIM} {what}, {variant} decode"
                word, guards, out, off = verdict(hs, fix, variant)
                assert word == golden[R.golden_key(codec, what, variant)], f"{w}: status {word:#x}"
                assert word != 0, f"{w}: a malformed block must be reported"
                assert guards, f"{w}: bytes outside the output were written"
                if variant == "plain":      # (a lane per block: the neighbours of the refused block are decoded as ever)
                    lo, hi = R.VICTIM * B, (R.VICTIM + 1) * B
                    assert np.array_equal(out[:lo], fix.data[:lo]) and np.array_equal(out[hi:], fix.data[hi:]), f"{w}: a neighbour of the malformed block differs"


@pytest.fixture(scope="module")
def hs():
    import torch

    assert torch.cuda.is_available(), "these tests need a GPU"
    import hsrle

    hsrle.lib()
    return hsrle


@pytest.mark.gpu
@pytest.mark.parametrize("codec, mixture", CASES, ids=ids)
def test_placed_runs(hs, codec, mixture):
    check_placed(hs, codec, mixture)


@pytest.mark.gpu
@pytest.mark.parametrize("codec, mixture", CASES, ids=ids)
def test_malformed_blocks_end_as_the_parent_said(hs, codec, mixture):
    check_malformed(hs, codec, mixture)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", (0, 1))
def test_forced_builds(flag):
    """-DHSRLE_DEC8_LAZY=0 / 1 builds of the library, where a developer has made them: every check above, in a child process that loads the build."""
    lib = os.path.join(REPO, "variants", f"libhsrle_dec8lazy{flag}.so")
    if not os.path.exists(lib):
        pytest.skip(f"no A/B build {os.path.relpath(lib, REPO)} (tools/build_variant_tu.sh inst_w8 dec8lazy{flag} -DHSRLE_DEC8_LAZY={flag})")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, HSRLE_LIB=lib), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "RUN_FILL_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


if __name__ == "__main__":
    # python tests/test_gpu_decode_run_fill.py [--record FILE]: every GPU check on the library HSRLE_LIB names (test_forced_builds), or the golden file from it
    sys.path.insert(0, os.path.join(REPO, "hypersonic-rle-kit_amd", "python"))
    import hsrle

    hsrle.lib()
    if "--record" in sys.argv:
        out = sys.argv[sys.argv.index("--record") + 1]
        json.dump(record_verdicts(hsrle), open(out, "w"), indent=1, sort_keys=True)
        print("recorded", out)
    else:
        for codec, mixture in CASES:
            check_placed(hsrle, codec, mixture)
            check_malformed(hsrle, codec, mixture)
        print("RUN_FILL_OK")
