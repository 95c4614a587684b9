"""The tables of ``f16_edge_cases.py`` without a GPU: the restated launch plans are self-consistent and describe what each case claims,
and every exact (tier A) case meets -- on its inputs and fp64 references alone -- the conditions under which
``test_f16_edges_gpu.py`` asserts bit equality: fp16-representable operands, per statistics tile sum y^2 < 2^24, per BST tile
sum |gz xhat| < 2^24 grid units, weight gradients 16 N H W < 2^24."""
import pytest
import torch

import f16_edge_cases as C
from conv_edge_helpers import conv3_64, dgrad3_64, fp16_exact, sums_exact, tap_conv3_64, tap_dgrad3_64, tile_sums

CUS = 256                     # the walk arithmetic is checked for an MI355X; the GPU test redoes it from the device's own count


def test_helpers_agree_with_the_full_references():
    """the one-tap references are the full fp64 convolutions of a kernel that is zero elsewhere; tile sums add up to the plane's"""
    R = C.IntRefs(2, 5, 7, 16, 4)
    for tap in (0, 4, 7, 8):
        wt = R.wt(tap)
        assert int((wt != 0).any(-1).any(-1).sum()) == 1
        assert torch.equal(tap_conv3_64(R.cpu("x"), wt[tap // 3, tap % 3], tap), conv3_64(R.cpu("x"), wt))
        R2 = C.IntRefs(2, 5, 7, 4, 16)
        assert torch.equal(tap_dgrad3_64(R2.cpu("gy"), R2.wt(tap)[tap // 3, tap % 3], tap), dgrad3_64(R2.cpu("gy"), R2.wt(tap)))
    y = R.ref("y")
    t = tile_sums(y, 4, 16)
    assert t.shape == (2, 2, 4) and torch.equal(t.sum(1), y.sum((1, 2)))
    assert fp16_exact(torch.tensor([2048.0, 0.25, 2.0 ** -24])) and not fp16_exact(torch.tensor([2049.0]))
    assert sums_exact(torch.full((1, 1, 1, 4), 3.0).double(), 1.0) and not sums_exact(torch.full((1, 1, 1, 4), 0.5).double(), 1.0)
    assert not sums_exact(torch.full((1, 2, 2, 1), 2.0 ** 22).double(), 1.0)


def test_per_tile_plan_is_self_consistent():
    for c in C.PER_TILE:
        n, h, w, ci, co, (rf, rd), legs, sd, sf, ks1 = c
        assert C.f16_supported(3, ci, co) and not C.fwd_p_eligible(n, h, w, ci, co)
        name, th, ntn = C.per_tile_row_f16(n, h, w, co, False)
        assert name == rf and (th, ntn) == {"h4": (4, 1), "nt1": (8, 1), "wg16": (16, 2), "wg8": (8, 2), "fall": (8, 1)}[name]
        if rd:
            assert C.f16_supported(3, co, ci) and not C.fwd_p_eligible(n, h, w, co, ci)
            assert C.per_tile_row_f16(n, h, w, ci, True)[0] == rd and rd in C.ROWS_DGRAD
        else:
            assert not C.f16_supported(3, co, ci) and not set(legs) & {"dgrad", "acc", "split"}
        if "cat" in legs:
            assert ci % 32 == 0
        for sp in sd:
            assert 0 < sp < ci and sp % 16 == 0 and (ci - sp) % 16 == 0
        for sp in sf:
            assert 0 < sp < co and sp % 16 == 0 and (co - sp) % 16 == 0
        assert ("split" in legs) == bool(sd or sf)
    assert {c[5][0] for c in C.PER_TILE} == C.ROWS_FWD and {c[5][1] for c in C.PER_TILE if c[5][1]} == C.ROWS_DGRAD


def test_persistent_plan_is_self_consistent():
    for c in C.PERSISTENT:
        n, h, w, ci, co, kind, inst_f, inst_d = c
        assert h != w and C.fwd_p_eligible(n, h, w, ci, co) and C.select_fwd_p_f16(h, ci, co) == inst_f
        assert h % inst_f[0] == 0 and ci == 16 * inst_f[2] and co % (16 * inst_f[1]) == 0
        assert C.fwd_p_eligible(n, h, w, co, ci) and C.select_fwd_p_f16(h, co, ci) == inst_d
        units = n * (h // 8) * (w // 16) * (co // 16)
        if kind == "edge":
            assert 1024 <= units < 1048
            legs = C.edge_legs(n, h, w, ci, co)
            assert ("cat" in legs) == (ci % 32 == 0) and ("dsc" in legs) == (co in (16, 32))
            for sp in C.persistent_splits(ci) if "split" in legs else ():
                assert 0 < sp < ci and sp % 16 == 0 and (ci - sp) % 16 == 0
                assert ci % (16 * C.select_fwd_p_f16(h, co, ci, sp)[1]) == 0 and sp % (16 * C.select_fwd_p_f16(h, co, ci, sp)[1]) == 0
        else:
            items, nz = n * (h // inst_f[0]) * (w // 16), co // (16 * inst_f[1])
            lens = C.walk_lengths(items, nz, CUS)
            assert items * nz > C.WG_PER_CU * CUS and min(lens) >= 2 and all(items % ipw for ipw in lens), (c, sorted(lens))
    for kind in ("edge", "walk"):
        assert {c[6] for c in C.PERSISTENT if c[5] == kind} == set(C.P_INSTANCES)


def test_wgrad_plan_is_self_consistent():
    for c in C.WGRAD:
        n, h, w, ci, co, forms, cas, what = c
        assert C.wgrad_f16_supported(n, h, w, ci, co)
        cit, cot, splits, tps, total = C.plan_wgrad_f16(n, h, w, ci, co)
        assert ci % (16 * cit) == 0 and co % (16 * cot) == 0 and total == n * (h // 8) * (w // 16)
        assert (splits - 1) * tps < total <= splits * tps, "every split holds a tile, together they hold all"
        if what == "one tile":
            assert total == 1
        elif what == "tile row":
            assert h == 8 and w > 16
        elif what == "tile column":
            assert w == 16 and h > 8
        else:
            assert tps > 1 and total % tps != 0 and total > 500
        for ca in cas:
            assert 0 < ca < ci and ca % 16 == 0
        assert bool(cas) == bool(set(forms) & {"cat", "sccat"})
    straddle = [c for c in C.WGRAD if any((s * C.plan_wgrad_f16(*c[:5])[3]) // ((c[1] // 8) * (c[2] // 16)) !=
                                          (min((s + 1) * C.plan_wgrad_f16(*c[:5])[3], C.plan_wgrad_f16(*c[:5])[4]) - 1) // ((c[1] // 8) * (c[2] // 16))
                                          for s in range(C.plan_wgrad_f16(*c[:5])[2]))]
    assert straddle, "a split whose tiles lie in two images"
    assert {C.wgrad_instance(c[3], c[4], f) for c in C.WGRAD for f in c[5]} == C.WGRAD_INSTANCES
    for shape in C.WGRAD_TIER_B:
        assert any(c[:5] == shape for c in C.WGRAD)


@pytest.mark.parametrize("case", C.PER_TILE, ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}" for c in C.PER_TILE])
def test_per_tile_cases_meet_the_exactness_conditions(case):
    n, h, w, ci, co, rows, legs, sd, sf, ks1 = case
    th = C.per_tile_row_f16(n, h, w, co, False)[1]
    R = C.IntRefs(n, h, w, ci, co)
    for tap in C.PER_TILE_TAPS[case[:5]]:
        C.conditions_a(R, legs, th, None, tap)
    if ks1:
        C.conditions_a(C.IntRefs(n, h, w, ci, co, ks=1), [l for l in legs if l in C.BASIC], th, None, -1)


@pytest.mark.parametrize("case", C.PERSISTENT, ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}-{c[5]}" for c in C.PERSISTENT])
def test_persistent_cases_meet_the_exactness_conditions(case):
    n, h, w, ci, co, kind, inst_f, inst_d = case
    R = C.IntRefs(n, h, w, ci, co)
    for tap in (C.TAPS if kind == "edge" else (-1,)):          # (the walks run the full kernel only)
        C.conditions_a(R, C.edge_legs(n, h, w, ci, co), inst_f[0], inst_d[0], tap)


@pytest.mark.parametrize("case", C.WGRAD, ids=[f"{c[0]}x{c[1]}x{c[2]}-{c[3]}to{c[4]}" for c in C.WGRAD])
def test_wgrad_cases_meet_the_exactness_conditions(case):
    n, h, w, ci, co, forms, cas, what = case
    C.wgrad_conditions_a(C.WgradRefs(n, h, w, ci, co, "A"), forms)
