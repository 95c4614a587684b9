"""CPU check that the cases of test_restail_gpu.py land in the launch regimes their ids name.

The regimes are chosen by host code (pick_chunk / slab_count / img_grid in csrc/norm.hip, SMSUT_EW_GRID_CAP in csrc/common.h): a
later change there can move a case into another regime, and the GPU tests would keep passing while the path they were written for
goes untested.  restail_ref.py restates that geometry; here its constants are compared with the sources and its chunk and slab
counts with the library (host-only queries: no compute entry point is called)."""
import ctypes

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import restail_ref as R
import test_instnorm_gpu as T


@pytest.fixture(scope="module")
def lib():
    ge.build()
    return ctypes.CDLL(ge.LIB)


def test_restated_constants_are_the_sources():
    assert R.parse_constants() == (R.EW_GRID_CAP, R.TPB, R.IN_SLAB_WGS)


def test_geometry_mirror_agrees_with_the_library(lib):
    for k, (n, h, w, c) in R.CASES:
        reg = R.regime(n, h, w, c)
        assert lib.smsut_in_chunks(n, h * w, c) == reg["chunks"], k
        assert lib.smsut_in_slabs(n, h * w, c) == reg["slabs"], k
        assert lib.smsut_amax_blocks(n, h * w, c) == reg["full"]["blocks"] * n, k


def test_every_case_sits_in_the_regime_its_id_names():
    reg = {k: R.regime(*s) for k, s in R.CASES}
    r = reg["one_chunk_tc1"]                     # the xor tree runs over all six levels
    assert r["fin_emit"] and r["tc"] == 1 and r["tree"] and r["slabs"] == 1 and r["vec"] == 4
    r = reg["one_chunk_256"]
    assert r["fin_emit"] and r["ppc"] == R.SHAPES["one_chunk_256"][1] * R.SHAPES["one_chunk_256"][2] == 256 and r["tree"]
    r = reg["vec1_two_chunks"]
    assert r["vec"] == 1 and r["chunks"] == 2 and r["last"] == 4 and not r["tree"] and r["tc"] == 6
    r = reg["cv3_general_walk"]
    assert r["cva"] == 3 and r["chunks"] == 3 and r["ragged"] and r["tc"] == 3 and not r["tree"]
    assert r["full"]["blocks"] == 7 and not r["full"]["aligned"] and not r["pooled"]["aligned"]
    r = reg["slabs4_tc6"]
    assert r["slabs"] == 4 and r["cv"] == 6 and r["tc"] == 6 and not r["tree"] and r["chunks"] == 2 and r["ragged"]
    r = reg["slabs_one_chunk"]
    assert r["slabs"] > 1 and r["fin_emit"] and r["tree"]
    r = reg["cap_two_trips"]
    assert r["full"] == dict(blocks=32, capped=True, aligned=True, trips=2, partial=True)
    r = reg["general_walk_two_trips"]
    assert r["full"]["capped"] and not r["full"]["aligned"] and r["full"]["trips"] == 2 and r["full"]["partial"]
    assert r["chunks"] > 1 and r["ragged"]
    r = reg["cap_pool_two_trips"]
    assert r["pooled"] == dict(blocks=16, capped=True, aligned=True, trips=2, partial=True)
    # the in-launch finalize of the backward needs several chunks and whole quads: some case of the tail tests has them, with and
    # without channel slabs
    fin = [k for k, s in R.TAIL_CASES if reg[k]["chunks"] > 1 and reg[k]["vec"] == 4]
    assert any(reg[k]["slabs"] > 1 for k in fin) and any(reg[k]["slabs"] == 1 for k in fin)
    # H != W wherever the plane is not one chunk: index formulas of the form pix / W, (h >> 1) * (W >> 1)
    for k, (n, h, w, c) in R.CASES:
        if reg[k]["chunks"] > 1 and k not in ("cap_two_trips",):
            assert h != w, k
    for hw_ in ((18, 30), (20, 24), (64, 72)):
        assert any(s[1:3] == hw_ for _, s in R.TAIL_POOL_CASES), hw_
    assert all(s[3] % 4 == 0 for _, s in R.TAIL_POOL_CASES) and any(s[3] % 4 for _, s in R.IN_POOL_CASES)
    assert [k for k, _ in R.CASES if k not in dict(R.TAIL_CASES)] == list(R.POOL_ONLY)


@pytest.mark.parametrize("name,shape", R.IN_POOL_CASES, ids=[k for k, _ in R.IN_POOL_CASES])
def test_statistics_bound_is_valid_for_the_seeds(name, shape):
    """the only data-dependent condition of the GPU tests: r < 0.5 of fwd_stat_bounds (asserted inside it), on the planes that
    test_instnorm_pool_fwd_bwd_vs_fp64 uses, with its seed and K = 1 (the partials are the exact sums rounded once)"""
    n, h, w, c = shape
    x = R.planes(n, h * w, c, R.IN_POOL_SEED)
    x64 = torch.from_numpy(x).double().view(n, h, w, c).permute(0, 3, 1, 2)
    dm, drel = T.fwd_stat_bounds(x64, 1, R.EPS)
    assert np.isfinite(dm).all() and np.isfinite(drel).all() and (drel < 1e-3).all()


@pytest.mark.parametrize("shape", R.TIE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tie_inputs_hold_enough_winning_pair_ties(shape):
    """the precondition of test_restail_pool_ties_are_first_wins_and_route_one_pixel: in the channels c % 3 == 1 more than
    TIE_MIN_PAIRS windows have positions 1 and 3 equal AND maximal (the forward restated in float32), and whole-window ties exist"""
    n, h, w, c = shape
    win = R.windows(R.fwd32(R.tie_inputs(shape, R.TIE_SEED), R.SLOPE), h, w)
    t0, t1 = np.arange(c) % 3 == 0, np.arange(c) % 3 == 1
    assert R.tie_pair_wins(win)[..., t1].sum() > 2 * R.TIE_MIN_PAIRS
    assert (win[:, :, :, t0, :] == win[:, :, :, t0, :1]).all()
