"""CPU checks of tests/block_ref.py, the fp64 reference that tests/test_block_fp64_gpu.py holds the fused BasicBlock to:

  1. with no masks given the restatement IS torch autograd of the ordinary F.leaky_relu / F.instance_norm / F.conv2d / F.max_pool2d
     composition, in every form (identity, conv shortcut, cat, pool with both / one gradient);
  2. the conditions that make the comparison flip-free hold for every case: min |pre-activation| >= MARGIN, MARGIN >= 20 d32 of the
     pre-activations, at most 1e-3 of a pool case's windows taken out as near-ties;
  3. the bars have teeth: the fp32 CPU replay passes ``block_ref.compare``, and five subtly wrong blocks fail it;
  4. every case lands in the kernel family and the plan its id names, and the list reaches every value of the plan's fields
     (``ops._block_plan`` / ``_block_bwd_plan`` on the library's host queries: no device is needed)."""
import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as ge
import block_ref as R

IDS = [c.id for c in R.CASES]


@pytest.fixture(scope="module")
def lib(request):
    """(ops, _hip) with the in-launch-finalize probe answered True, as on a device outside a foreign stream capture"""
    ge.build()
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip, ops
    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "_fin_available", lambda like: True)
    request.addfinalizer(mp.undo)
    assert not ops.CONV_F16 and not ops._PAIR_FWD and ops.FIN_ON
    return ops, _hip


# ------------------------------------------------------------------------------------------------------------------- 1. the reference
def torch_block(c, t, grads):
    """the ordinary composition, differentiated by autograd"""
    leaf = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    x = leaf["x"] if "x" in leaf else torch.cat([leaf["xa"], leaf["xb"]], 1)
    y = F.leaky_relu(F.instance_norm(F.conv2d(x, leaf["w1"], padding=1), weight=leaf["g1"], bias=leaf["b1"], eps=R.IN_EPS), c.slope)
    y = F.instance_norm(F.conv2d(y, leaf["w2"], padding=1), weight=leaf["g2"], bias=leaf["b2"], eps=R.IN_EPS)
    idn = F.instance_norm(F.conv2d(x, leaf["ws"]), weight=leaf["gs"], bias=leaf["bs"], eps=R.IN_EPS) if c.has_sc else x
    out = F.leaky_relu(y + idn, c.slope)
    pooled = F.max_pool2d(out, 2) if c.pool else None
    outs, gs = [out], [grads["gout"]]
    if c.pool:
        outs, gs = {"both": ([out, pooled], [grads["gout"], grads["gpooled"]]), "pooled": ([pooled], [grads["gpooled"]]), "skip": ([out], gs)}[c.grads]
    res = dict(zip(leaf, torch.autograd.grad(outs, list(leaf.values()), gs)))
    res.update(out=out.detach(), pooled=None if pooled is None else pooled.detach())
    return res


@pytest.mark.parametrize("cid", ["tile-identity", "tile-identity-relu", "tile-sc-tails", "cat-materialised", "wino-sc-1image", "pool-both-tile",
                                 "pool-only-pooled-tile", "pool-only-skip-tile"])
def test_reference_is_torch_autograd_when_no_mask_is_given(cid):
    c = R.case(cid)
    t, grads, masks, _ = R.make_inputs(c)
    own = {}
    got = R.step(c, t, grads, own, torch.float64)
    assert set(own) == {"act1", "out"} and all(torch.equal(own[k], masks[k]) for k in own)      # filled from the run's own pre-activations
    want = torch_block(c, t, grads)
    for k in ["out"] + (["pooled"] if c.pool else []) + R.grad_names(c):
        e = R.rel_err(got[k].numpy(), want[k].numpy())
        assert e < 1e-12, (k, e)
    assert set(R.grad_names(c)) == set(t)


def test_activation_uses_a_given_mask():
    c = R.case("tile-identity")
    t, grads, masks, _ = R.make_inputs(c)
    flipped = {"act1": ~masks["act1"], "out": masks["out"]}
    a, b = R.step(c, t, grads, masks, torch.float64), R.step(c, t, grads, flipped, torch.float64)
    assert R.rel_err(b["out"].numpy(), a["out"].numpy()) > 1e-2


# ------------------------------------------------------------------------------------------------------------------- 2. the conditions
@pytest.mark.parametrize("cid", IDS)
def test_case_is_flip_free(cid, lib):
    ops, H = lib
    c = R.case(cid)
    ref = R.reference(c)
    p, b = R.plans(ops, c, torch.empty(R.like_shape(c), device="meta"))
    i = ref.info
    print(f"{cid}: MARGIN {R.MARGIN:.3g}  min |pre| {i['margin']:.3g}  d32(pre) {i['pre_d32']:.3g} (abs {i['pre_d32_abs']:.3g})  "
          f"zeroed windows {i['zeroed']:.3g}  regime {R.regime_of(H, c)}  {p}  {b}")
    assert i["margin"] >= R.MARGIN
    assert R.MARGIN >= R.MARGIN_OVER_D32 * i["pre_d32"]
    assert i["zeroed"] <= R.MAX_ZEROED_WINDOWS
    for k in ("act1", "out"):                            # both signs occur at both sites: a mask of one value would test nothing
        assert 0.05 < float(ref.masks[k].double().mean()) < 0.95, k
    for v in list(ref.t.values()) + list(ref.grads.values()):          # every input is an fp32 value: the device gets the same numbers
        assert torch.equal(v, v.float().double()) and not v.requires_grad
    if c.pool:
        assert c.slope > 0 and float(ref.grads["gpooled"].abs().max()) > 0
        # outside the windows taken out, the fp32 replay pools the position the fp64 run pools
        at32 = F.max_pool2d(ref.r32["out"], 2, return_indices=True)[1]
        at64 = F.max_pool2d(ref.r64["out"], 2, return_indices=True)[1]
        assert torch.equal(at32 != at64, (at32 != at64) & (R.window_top2_gap(ref.r64["pre2"]) < R.MARGIN))


def test_margin_is_the_smallest_half_gap_of_the_list_rounded_down():
    least = min(R.reference(c).info["margin"] for c in R.CASES)
    assert R.MARGIN <= least < 1.1 * R.MARGIN, least


# ------------------------------------------------------------------------------------------------------------------- 3. teeth
@pytest.mark.parametrize("cid", R.TEETH_CASES)
def test_fp32_replay_passes_and_wrong_blocks_fail(cid):
    """the fp32 CPU restatement stands in for the device.  It passes max(4 d32, floor) trivially; each wrong block must miss it."""
    c = R.case(cid)
    ref = R.reference(c)
    names = ["out"] + R.grad_names(c)
    assert R.compare(f"{cid} fp32 replay", R.rows_of(c, ref.r32, ref, names)) == []
    for wrong in R.CORRUPTIONS:
        got = R.step(c, ref.t, ref.grads, ref.masks, torch.float32, corrupt=wrong)
        fails = R.compare(f"{cid} {wrong}", R.rows_of(c, got, ref, names))
        assert fails, f"{wrong} passes the comparison: the bar or the norm is too weak"
        hit = {"act1_bit": "x", "stats2_row": "out", "dx_sc_image": "x", "w1_border_row": "w1", "g2_image": "g2"}[wrong]
        assert hit in [f[0] for f in fails], (wrong, fails)
        if wrong in ("dx_sc_image", "w1_border_row", "g2_image"):       # one tensor is wrong, and only that one is named
            assert [f[0] for f in fails] == [hit], (wrong, fails)


# ------------------------------------------------------------------------------------------------------------------- 4. coverage
def test_every_case_lands_where_its_id_says(lib):
    ops, H = lib
    seen = {}
    for c in R.CASES:
        p, b = R.plans(ops, c, torch.empty(R.like_shape(c), device="meta"))
        seen[c.id] = (p, b)
        r1, r2 = R.regime_of(H, c)
        assert r2 == c.regime, (c.id, r1, r2)
        # conv1 runs the same family, except on 8 input channels (the tap-paired direct form of the resident kernel)
        assert r1 == (c.regime if c.ci != 8 else "res_direct"), (c.id, r1, r2)
        assert (p.has_sc, p.pool, p.virtual, p.cat is not None) == (c.has_sc, c.pool, c.form == "cat", c.form in ("cat", "catmat")), c.id
        assert not (p.f16a or p.f16 or p.hs or p.pair or b.nb or b.f16w1 or b.f16w2 or b.fused_wsc16 or b.fused_dsc16), c.id
        tile = c.regime == "tile"
        assert (p.inaff, b.pers2) == (not tile, not tile), c.id
        assert b.tail == ("pool" if c.pool and c.grads == "both" else "fin" if c.has_sc else "plain"), c.id
        assert (b.dx is None) == (c.needs == "no_x"), c.id
        f, g = R.expected_launches(H, p, b, c.pool and c.grads == "pooled")
        assert all(k in H.SIGNATURES for k in f + g), c.id
        assert (g[0] == "smsut_maxpool2_bwd") == c.id.startswith("pool-only-pooled"), c.id

    def P(cid):
        return seen[cid][0]

    def B(cid):
        return seen[cid][1]
    # per-tile kernels: a1 is built, every statistics set has its own finalize, the data gradient of conv2 is conv + instnorm_bwd
    c = R.case("tile-identity")
    assert c.w % 16 and not P(c.id).fused_sc and B(c.id).dx == "accum" and B(c.id).tail == "plain"
    c = R.case("tile-sc-tails")
    assert c.ci % 16 and c.co % 16 and c.h % 2 and c.w % 2 and not P(c.id).fused_sc and B(c.id).dx == "accum" and not B(c.id).fused_wsc
    # the shortcut's data gradient as the k = 1 MFMA conv: only beyond the streaming 1x1 kernel's 512 reduction channels
    c = R.case("tile-sc-k1")
    assert not H.call("smsut_conv1x1_supported", c.co, c.ci) and B(c.id).dx == "accum_k1"
    assert H.call("smsut_conv1x1_supported", c.ci, c.co) and B("tile-sc-1x1").dx == "accum"
    # streamed Winograd: identity -> inaff without fin; conv shortcut -> every statistics set finalised in its launch
    assert not P("wino-identity").fin and not B("wino-identity").fin_b
    p, b = seen["wino-sc-1tile"]
    assert (p.fused_sc, p.fin, p.t3, p.t3b, b.fin_b, b.fused_wsc) == (True, True, 1, 1, True, True)
    p, b = seen["wino-sc-1image"]
    assert (p.n, p.fused_sc, p.fin, p.t3, p.t3b, b.fin_b) == (1, True, True, 6, 6, True) and p.ci > p.co
    # resident kernels: exactly the size floor; the direct form; a workgroup's items span several images
    c = R.case("res-wino-16")
    assert c.n * (c.h // 8) * (c.w // 16) * (c.co // 16) == 1024
    c = R.case("res-direct-32")
    assert c.h % 16 and P(c.id).fin and B(c.id).fused_wsc and B(c.id).fin_b
    c = R.case("res-many-images")
    assert c.h == 8 and c.n >= 256 and P(c.id).t3 == c.w // 16
    assert R.case("first-block").ci == 8 and B("first-block").dx == "sc" and P("first-block").fused_sc
    # cat forms: the block-input gradient goes into the two parts
    assert B("cat-virtual-32").dx == "sc" and B("cat-virtual-64").dx == "split" and B("cat-materialised").dx == "split"
    assert P("cat-virtual-32").fused_sc and P("cat-virtual-64").fused_sc and not P("cat-materialised").fused_sc
    for cid in ("tile-sc-1x1", "res-direct-32"):
        assert seen[cid][1]._replace(dx=None) == seen[cid + "-no-x"][1] and seen[cid] == seen[cid + "-frozen"]

    # over the whole list every value of every fp32 field occurs (none is unreachable in fp32: ``accum_k1`` needs Cout > 512, which
    # no network of the project has, and is reached by tile-sc-k1)
    def values(get):
        return {get(*pb) for pb in seen.values()}
    for field in ("fused_sc", "fin", "inaff"):
        assert values(lambda p, b: getattr(p, field)) == {True, False}, field
    assert True in values(lambda p, b: p.virtual)
    assert values(lambda p, b: b.tail) == {"pool", "fin", "plain"}
    for field in ("pers2", "fin_b", "fused_wsc"):
        assert values(lambda p, b: getattr(b, field)) == {True, False}, field
    assert values(lambda p, b: b.dx) == {None, "sc", "split", "accum", "accum_k1"}


def test_tail_backward_without_the_finalize_probe_is_plain(lib):
    """the probe decides ``fin`` / ``fin_b`` / the tail's form and nothing else: inside a foreign stream capture the same cases keep the
    separate finalize launches"""
    ops, H = lib
    c = R.case("res-direct-32")
    like = torch.empty(R.like_shape(c), device="meta")
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "_fin_available", lambda like: False)
        p, b = R.plans(ops, c, like, fin=False)
    assert (p.fused_sc, p.fin, p.inaff, b.tail, b.fin_b, b.pers2) == (True, False, True, "plain", False, True)
    f, g = R.expected_launches(H, p, b)
    assert "smsut_in_finalize_fwd2" in f and "smsut_in_finalize_bwd" in g and not [k for k in f + g if k.endswith("_fin")]
