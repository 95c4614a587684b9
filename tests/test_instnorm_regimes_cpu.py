"""CPU check that the cases of test_instnorm_gpu.py still land in the InstanceNorm reduction regimes they are named after.

The regimes are chosen by host code (pick_chunk / slab_count in csrc/norm.hip, the tile selection of the persistent convs): a later
change there can move a case into another regime, and the GPU tests would keep passing while the path they were written for goes
untested.  Host-only queries, like test_cabi_cpu.py: no compute entry point is called."""
import ctypes

import pytest

import __graft_entry__ as ge
import test_instnorm_gpu as T


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return ctypes.CDLL(ge.LIB)


def test_chunk_mirror_agrees_with_the_library(lib):
    """in_regime() (the tests' copy of pick_chunk and slab_count) is what the library does: the regimes below and the accumulation
    bounds of the GPU tests are derived from it"""
    shapes = [(n, h * w, c) for _, (n, c, h, w) in T.FWD_CASES + T.BWD_CASES] + [(n, h * w, c) for n, c, h, w in T.EDGE_SHAPES]
    shapes += [s for _, s in T.TAIL_FIN_CASES]
    for n, hw, c in shapes:
        _, chunks, slabs, _ = T.in_regime(n, c, hw)
        assert lib.smsut_in_chunks(n, hw, c) == chunks, (n, hw, c)
        assert lib.smsut_in_slabs(n, hw, c) == slabs, (n, hw, c)


def _regime(n, c, hw):
    _, chunks, slabs, vec = T.in_regime(n, c, hw)
    return chunks, slabs, vec


@pytest.mark.parametrize("table", ["FWD_CASES", "BWD_CASES"])
def test_statistics_cases_cover_every_regime(lib, table):
    cases = dict(getattr(T, table))
    reg = {k: _regime(n, c, h * w) for k, (n, c, h, w) in cases.items()}
    hit = {
        "one_chunk_vec4": [k for k, (ch, _, v) in reg.items() if ch == 1 and v == 4],
        "one_chunk_vec1": [k for k, (ch, _, v) in reg.items() if ch == 1 and v == 1],
        "2_16_ragged": [k for k, (ch, _, _) in reg.items() if 2 <= ch <= 16 and (lambda s: s[2] * s[3] % T.pick_chunk(s[2] * s[3], s[1], s[0]))(cases[k])],
        "exactly_16": [k for k, (ch, _, _) in reg.items() if ch == 16],
        "exactly_17": [k for k, (ch, _, _) in reg.items() if ch == 17],
        "17_255": [k for k, (ch, _, _) in reg.items() if 17 < ch < 256],
        "exactly_256": [k for k, (ch, _, _) in reg.items() if ch == 256],
        "over_256": [k for k, (ch, _, _) in reg.items() if ch > 256],
        "over_256_ragged_round": [k for k, (ch, _, _) in reg.items() if ch > 256 and ch % 256],
        "slabs": [k for k, (_, z, _) in reg.items() if z > 1],
        "vec1_multi_chunk": [k for k, (ch, _, v) in reg.items() if ch > 1 and v == 1],
    }
    for name, ks in hit.items():
        assert ks, f"no case of {table} is in the regime {name}"
    for c in (12, 20, 24, 96):                   # channel counts that are not powers of two (img_walk's li % CV branch)
        assert any(s[1] == c for s in cases.values()), c
    for n in (16, 32):                           # the production grid-stride walks at 256 x 256
        assert any(s[0] == n and s[2:] == (256, 256) for s in cases.values()), n
    # the named regimes are the ones the names promise
    for k, (ch, z, v) in reg.items():
        if k.startswith("chunks_"):
            assert ch == int(k.split("_")[1]), (k, ch)
        if k.startswith("one_chunk"):
            assert ch == 1 and (v == 1) == ("vec1" in k), (k, ch, v)
        if k.startswith("slabs_"):
            assert z == int(k.split("_")[1]), (k, z)


def test_conv_finalize_cases_cover_the_tile_counts(lib):
    tiles, cat_tiles, forms = {}, set(), set()
    for k, (n, h, w, ci, co) in T.CONV_FIN_CASES:
        assert lib.smsut_conv2d_fwd_sc_supported(n, h, w, ci, co, 0) == 1, k
        if T.conv_fin_cat(ci):                   # the virtual-cat leg of the fused shortcut conv runs (and asserts this too)
            assert lib.smsut_conv2d_fwd_sc_supported(n, h, w, ci, co, 1) == 1, k
        assert lib.smsut_conv2d_mfma_persistent(n, h, w, ci, co, 3, 0) == 1, k
        assert lib.smsut_conv2d_mfma_persistent(n, h, w, co, co, 3, 0) == 1, k
        t1 = lib.smsut_conv2d_mfma_tiles(n, h, w, ci, co, 3, 0)
        t2 = lib.smsut_conv2d_mfma_tiles(n, h, w, co, co, 3, 0)
        assert t1 == t2 == int(k.split("_")[1].split("-")[0]), (k, t1, t2)
        tiles[k] = (t1, n, co)
        if T.conv_fin_cat(ci):
            cat_tiles.add(t1)
        forms |= {lib.smsut_conv2d_mfma_form(n, h, w, ci, co, 0), lib.smsut_conv2d_mfma_form(n, h, w, co, co, 0)}
    got = {t for t, _, _ in tiles.values()}
    for counts in (got, cat_tiles):              # every tile count, and again with the virtual-cat input
        for want in (1, 5, 16, 17):
            assert want in counts, want
        assert counts & {2, 3}
        assert any(t > 256 and t % 256 for t in counts)
    # every kernel family that finalises in the launch: direct and resident-weight Winograd (conv_mfma.hip), streamed-weight
    # Winograd (conv_wino.hip)
    assert forms == {0, 1, 2}, forms
    # a workgroup walks several images: one tile per image and more (image, 16-output-channel) items than the grid has workgroups.
    # The grid is one resident round: 256 CUs (MI355X) x at most 8 workgroups of 256 threads per CU (32 waves of a CU's 4 SIMDs)
    # = 2048 workgroups at the most, so more than 2048 items give every workgroup at least two images.
    assert any(t == 1 and n * (co // 16) > 256 * 8 for t, n, co in tiles.values())


def test_restail_finalize_cases_cover_the_chunk_counts(lib):
    got = {lib.smsut_in_chunks(n, hw, c) for _, (n, hw, c) in T.TAIL_FIN_CASES}
    for want in (1, 5, 16, 17):
        assert want in got, want
    assert got & {2, 3}
    assert any(ch > 256 and ch % 256 for ch in got)
    for _, (n, hw, c) in T.TAIL_FIN_CASES:
        assert c % 4 == 0                        # the in-launch form (whole channel quads)
