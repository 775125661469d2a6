"""tests/decoder_fixtures.py keeps its promises, for all 110 codecs and without a GPU: the ratios that decide the decoder's stream ring, the make-up
of every wave, a partial last block that ends off a 16-byte boundary, streams the oracle itself decodes back to the blocks -- and the ring the
library says such a container takes (hsrle_decode_ring needs no device), so that the GPU tests in test_gpu_decode_variants.py run the kernels
they name.

Bounds (fixed before the fixture was written, from the thresholds 0.215 / 0.25 of the ring rule with room to spare): sparse (payload + 32) / U <= 0.18,
dense >= 0.40, at B = 4096 (3 waves) and B = 16384 (70 blocks)."""
import struct

import pytest

import decoder_fixtures as F
from hsrle_testlib import CODECS

SPARSE_MAX, DENSE_MIN = 0.18, 0.40


@pytest.fixture(scope="module")
def hs():
    import hsrle

    hsrle.lib()
    return hsrle


@pytest.mark.parametrize("codec", CODECS, ids=lambda c: c.key)
def test_fixture_conditions(hs, oracle, codec):
    for B, blocks in ((4096, 192), (16384, 70)):
        for layout in ("sparse", "dense"):
            f = F.fixture(codec, layout, B)
            what = f"{codec.key} {layout} B {B}"
            assert len(f.kinds) == len(f.streams) == blocks and f.U == (blocks - 1) * B + B // 2 + 5 and f.U % 16 != 0 and f.U % B != 0, what
            ratio = (sum(len(s) for s in f.streams) + 32) / f.U
            assert ratio == f.ratio and (ratio <= SPARSE_MAX if layout == "sparse" else ratio >= DENSE_MIN), f"{what}: ratio {ratio:.4f}"
            # every full wave (64 consecutive blocks = one workgroup of the block decoder) holds the layout's mixture -- what the blocks CONTAIN is checked below; the
            # 70-block container's second wave is the first six blocks of another shuffle, whatever they are
            want = dict(F.LAYOUTS[layout])
            for w in range(blocks // 64):
                kinds = f.kinds[64 * w : 64 * w + 64]
                assert {k: kinds.count(k) for k in want} == want, what
                assert kinds.count("L") >= 2 and kinds.count("D") >= 2
            # the container is what include/hsrle.h lays out, the streams decode (by the oracle) to the blocks they were made from
            head = struct.unpack_from("<8sIIQIIQQ", f.container, 0)
            assert head == (b"HSRLEKIT", 1, CODECS.index(codec), f.U, B, blocks, f.payload_size, len(f.container)), what
            table = struct.unpack_from(f"<{blocks + 1}Q", f.container, 64)
            p0 = 64 + 8 * (blocks + 1)
            assert table[0] == 0 and table[-1] == f.payload_size and f.container[p0 + f.payload_size :] == bytes(32), what
            data = f.data.tobytes()
            for b, s in enumerate(f.streams):
                assert f.container[p0 + table[b] : p0 + table[b + 1]] == s
                block = data[b * B : (b + 1) * B]
                assert oracle.decompress(codec, s, len(block)) == block, f"{what}: block {b} ({f.kinds[b]})"
            # the kind of a block is what it says: Z is one symbol, L compresses to more than the block, the others to less, D is a dense packet chain
            for b in range(blocks - 1):
                block, kind = data[b * B : (b + 1) * B], f.kinds[b]
                if kind == "Z":
                    assert block == (block[: codec.S] * (B // codec.S + 1))[:B] and len(f.streams[b]) < 48 + 2 * codec.S, what   # (a header, one run packet, the terminator)
                if kind == "L":
                    assert len(f.streams[b]) > B, what
                if kind in "DMV":
                    assert len(f.streams[b]) < B, f"{what}: block {b} ({kind}) is stored as literals"
                if kind == "D":
                    # packet-dense: a run packet for at most every (R + 2) symbols (counted by the oracle's decoder); 8 bit symbols: more packets than the split
                    # decode's packet list holds (B / 8 + 2 entries), so the walking lane closes the list and finishes the block itself
                    packets = oracle.run_packets(codec, f.streams[b], B)
                    assert packets >= F.dense_packets_min(codec, B) > B // (12 * codec.S), f"{what}: block {b} has {packets} run packets"
                    assert codec.S > 1 or packets > B // 8 + 2, f"{what}: block {b} has {packets} run packets, its packet list holds {B // 8 + 2}"
            assert hs.decode_ring(codec.key, f.U, f.payload_size) == F.expected_ring(f) == (64 if layout == "sparse" and codec.S <= 4 else 128), what


def test_fixtures_are_deterministic_and_the_front_blocks_do_not_depend_on_the_tail():
    codec = CODECS[1]
    a, ka = F.build_input(codec, "dense", 4096)
    b, kb = F.build_input(codec, "dense", 4096)
    assert a.tobytes() == b.tobytes() and ka == kb
    c, kc = F.build_input(codec, "dense", 4096, blocks=65, last_len=17, last_kind="L")
    d, kd = F.build_input(codec, "dense", 4096, blocks=65, last_len=129, last_kind="Z")
    assert c.size == 64 * 4096 + 17 and d.size == 64 * 4096 + 129 and c[: 64 * 4096].tobytes() == d[: 64 * 4096].tobytes() and kc[:-1] == kd[:-1]
    assert kc[-1] == "L" and kd[-1] == "Z" and len(set(d[64 * 4096 :].tolist())) == 1
    with pytest.raises(AssertionError):
        F.build_input(codec, "sparse", 1024)          # too close to 0.215: not built
