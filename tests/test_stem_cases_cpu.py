"""The tables of ``stem_cases.py`` without a GPU: every claim of the case table follows from the restated launch plan, the restated
predicate agrees with ``is_stem`` of ``test_conv_families_gpu.py``, every integer case meets -- on its operands and fp64 references
alone -- the conditions under which ``test_stem_edges_gpu.py`` asserts bit equality, and the one-hot references are the fp64
convolutions of ``conv_edge_helpers.conv_ref``."""
import pytest
import torch

import stem_cases as C
from conv_edge_helpers import conv_ref, gen, rn
from test_conv_families_gpu import is_stem


@pytest.mark.parametrize("cid", list(C.ALL))
def test_plan_claims_hold(cid):
    C.assert_claims(cid)


def test_the_cases_reach_every_workgroup_walk():
    """tiles per workgroup 1, 2 and 3; a short last workgroup of one and of two tiles; a workgroup inside one image and across two"""
    plans = {cid: C.StemPlan(*C.STEM[cid]) for cid in C.STEM}
    assert {p.tpw for p in plans.values()} == {1, 2, 3}
    assert {len(p.tiles(p.nwg - 1)) for p in plans.values() if p.tpw > 1} == {1, 2}
    for cid in ("E", "F"):
        p = plans[cid]
        assert {len(p.images(g)) for g in range(p.nwg)} == {1, 2}
        assert sorted(t for g in range(p.nwg) for t in p.tiles(g)) == list(range(p.total)), "the workgroups partition the tiles"
        n, h, w = C.STEM[cid]
        for ci in C.CINS:                                       # the workspace query of the general plan holds the stem kernel's slabs
            assert p.nwg * 25 * ci * 8 <= C.flat_ws(n, h, w, ci)
    assert set(C.ONE_HOT_SHAPES) <= set(C.STEM)


def test_the_slab_cap_cannot_bind_on_a_stem_shape():
    """a 16 x 64 stem tile is 2 x 4 tiles of flat_plan, whose split count therefore exceeds min(total, 512): stem_wgrad_wgs' second
    clamp is dead for every stem shape (swept here over tile counts round both caps)"""
    for n in list(range(1, 40)) + [63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4096, 5000]:
        for h, w in ((16, 64), (48, 64), (16, 320), (32, 128)):
            p = C.StemPlan(n, h, w)
            assert p.slabs >= min(p.total, C.STEM_WGS) == p.wgs


def test_predicate_agrees_with_the_conv_families_restatement():
    for h in (8, 16, 24, 32, 48):
        for w in (32, 64, 96, 128, 192, 320):
            for ci in (1, 2, 5, 8):
                for co, k, s, p in ((8, 5, 1, 2), (4, 5, 1, 2), (8, 3, 1, 1), (8, 5, 2, 2), (8, 5, 1, 1)):
                    assert C.stem_shape(h, w, ci, co, k, s, p) == is_stem(h, w, ci, co, k, s, p), (h, w, ci, co, k, s, p)
    for cid, (n, h, w) in C.ALL.items():
        for ci in C.CINS:
            assert is_stem(h, w, ci, 8, 5, 1, 2) == (cid in C.STEM)


@pytest.mark.parametrize("ci", C.CINS)
@pytest.mark.parametrize("cid", list(C.ALL))
def test_integer_cases_meet_the_exactness_conditions(cid, ci):
    ops = C.integer_operands(cid, ci)
    assert C.asymmetric(ops["w"])
    C.integer_conditions(ops, C.refs64(ops), C.abs_refs64(ops))
    nb, anb = C.refs64(ops, bias=False), C.abs_refs64(ops, bias=False)
    assert C.sums_exact(nb["y"], 0.125, 1, 1) and C.sums_exact(anb["y"], 0.125, 1, 1)


@pytest.mark.parametrize("cid", ["A", "nearH"])
def test_references_agree_with_conv_ref(cid):
    """the three fp64 references of this module against the autograd reference of the other convolution edge tests"""
    for ci in C.CINS:
        ops = C.integer_operands(cid, ci)
        r = C.refs64(ops)
        ry, rgx, rgw, _ = conv_ref(ops["x"], ops["w"], ops["b"], 1, 2, ops["gy"])
        assert torch.equal(r["y"], ry) and torch.equal(r["gx"], rgx) and torch.equal(r["gw"], rgw)
        assert torch.equal(C.refs64(ops, bias=False)["y"], conv_ref(ops["x"], ops["w"], None, 1, 2))
        fo = C.float_operands(cid, ci)                          # Gaussian operands: the two fp64 sums differ in order only
        r, a = C.refs64(fo), C.abs_refs64(fo)
        terms = (25 * ci + 1, 200, fo["x"].shape[0] * fo["x"].shape[1] * fo["x"].shape[2])      # K of each sum: 2 (K + 2) 2^-53 A apart
        for got, ref, scale, k in zip((r["y"], r["gx"], r["gw"]), conv_ref(fo["x"], fo["w"], fo["b"], 1, 2, fo["gy"]),
                                      (a["y"], a["gx"], a["gw"]), terms):
            assert bool(((got - ref).abs() <= 2 * (k + 2) * 2.0 ** -53 * scale).all())


@pytest.mark.parametrize("ci", C.CINS)
@pytest.mark.parametrize("cid", C.ONE_HOT_SHAPES)
def test_one_hot_references_are_the_fp64_convolutions(cid, ci):
    n, h, w = C.ALL[cid]
    g = gen(90 + ci)
    x, gy = rn(g, n, h, w, ci), rn(g, n, h, w, C.CO)
    taps = C.one_hot_taps(ci)
    assert len(taps) == 25 * ci * 2 and len(set(taps)) == len(taps)
    for kh, kw, c, co in taps:
        wt = C.one_hot_weight(kh, kw, c, co, ci)
        assert float(wt.sum()) == 1.0 and int((wt != 0).sum()) == 1
        ry, rgx, _, _ = conv_ref(x, wt, None, 1, 2, gy)
        assert torch.equal(C.one_hot_fwd_ref(x, kh, kw, c, co).double(), ry), (kh, kw, c, co)
        assert torch.equal(C.one_hot_dgrad_ref(gy, kh, kw, c, co, ci).double(), rgx), (kh, kw, c, co)
    pixels = C.one_hot_pixels(cid)
    assert {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)} <= {(y, xx) for _, y, xx in pixels}
    assert {(0, c) for c in range(60, min(68, w))} <= {(y, xx) for _, y, xx in pixels}
    if cid == "B":
        assert {(15, 63), (16, 64), (15, 64), (16, 63)} <= {(y, xx) for _, y, xx in pixels} and {i for i, _, _ in pixels} == {0, 1}
    for n0, y, xx in pixels:
        for co in C.ONE_HOT_CO:
            _, _, rgw, _ = conv_ref(x, torch.zeros(5, 5, ci, C.CO), None, 1, 2, C.one_hot_gy(cid, n0, y, xx, co))
            assert torch.equal(C.one_hot_wgrad_ref(x, n0, y, xx, co).double(), rgw), (n0, y, xx, co)


def test_dense_one_hot_operands_have_full_mantissas():
    """the point of the one-hot family: values a narrower type could not carry (fp16 / bf16 / tf32 keep at most 11 of the 24 bits)"""
    x = rn(gen(91), 2, 32, 128, 5)
    assert float((x.half().float() != x).float().mean()) > 0.99 and float((x.bfloat16().float() != x).float().mean()) > 0.99
    low13 = x.view(torch.int32) & 0x1FFF                         # the 13 bits tf32 drops
    assert float((low13 != 0).float().mean()) > 0.99
