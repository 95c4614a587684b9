"""CPU checks of tests/block_f16_ref.py, the fp16 rounding model and the cases tests/test_block_f16_gpu.py holds the fp16-operand fused
BasicBlock to fp64 with:

  1. every case lands on the plan branch it claims (``ops._block_plan`` / ``_block_bwd_plan`` under fp16, host queries only), the list
     reaches every fp16 value of the plan's fields, and the launch list of every plan names entry points of the library;
  2. with no rounding switched on the model IS ``block_ref.step(..., torch.float32)``, bit for bit, and with the plan's roundings on it
     sits where fp16 rounding puts it: a few 1e-4 from fp64, not on the fp32 floor and not at 1e-2;
  3. the conditions that keep discrete events out of the comparison, for every case they apply to: sign cases have
     min |pre-activation| >= 6 x max |model pre-activation - fp64 pre-activation|; pool cases lose at most 3 % of their windows;
  4. the bars have teeth: the model passes them, and each subtly wrong block -- block_ref's five and a gradient operand converted to
     fp16 without its scale -- misses at least one."""
import pytest
import torch

import block_f16_ref as M
import block_ref as R

IDS = [c.id for c in M.F16_CASES]


def ref_of(c):
    p, b = M.plans_cpu(c)
    return M.reference(c, M.flags_of(p, b))


def names_of(c):
    skip = ("x", "xa", "xb") if c.needs == "no_x" else ("w1", "ws") if c.needs == "frozen" else ()
    return ["out"] + (["pooled"] if c.pool else []) + [k for k in R.grad_names(c) if k not in skip]


# ------------------------------------------------------------------------------------------------------------------- 1. the plans
def test_every_case_lands_on_the_branch_it_claims():
    from smsut_amd import _hip as H
    from smsut_amd import ops
    before = ops.conv_dtype()
    seen = {}
    for c in M.F16_CASES:
        p, b = seen[c.id] = M.plans_cpu(c)
        print(f"{c.id}: {p}\n{c.id}: {b}\n{c.id}: {M.flags_of(p, b)}")
        M.check_plan(c, p, b)
        f, g = R.expected_launches(H, p, b, c.pool and c.grads == "pooled")
        assert all(k in H.SIGNATURES for k in f + g), c.id
        assert (g[0] == "smsut_maxpool2_bwd") == (c.pool and c.grads == "pooled"), c.id
        assert (c.slope == 1.0) == (c.branch != "sign"), c.id
    assert ops.conv_dtype() == before                    # the conv dtype was put back
    assert M.plans_cpu(M.case(M.FP32_TWIN_CASE))[0].hs

    def values(get):
        return {get(*pb) for pb in seen.values()}
    for field in ("f16a", "hs", "fused_sc", "virtual", "pool", "has_sc"):
        assert values(lambda p, b: getattr(p, field)) == {True, False}, field
    assert values(lambda p, b: b.tail) == {"pool", "hs", "amax"}
    for field in ("amax1", "pers2", "f16w1", "f16w2", "fused_wsc16", "fused_wsc", "fused_dsc16"):
        assert values(lambda p, b: getattr(b, field)) == {True, False}, field
    assert values(lambda p, b: b.dx) == {None, "sc_f16", "sc", "split", "accum"}
    assert {c.ci for c in M.F16_CASES if M.plans_cpu(c)[0].hs} >= {8, 16, 32, 64}         # every reduction width of the persistent kernel
    # the needs variants of the fully fused case: no_x drops the fused data-gradient, and with it the reason the scale is joint stays
    # the fused weight gradient alone; frozen changes no decision
    full, nox, frz = (seen[k][1] for k in ("hs-32-32", "hs-32-32-no-x", "hs-32-32-frozen"))
    assert nox == full._replace(fused_dsc16=False, dx=None) and frz == full
    assert M.flags_of(*seen["hs-32-32-no-x"]).joint and not M.flags_of(*seen["hs-32-32-no-x"]).dsh
    # ``basic_block`` passes eleven arguments, so autograd's ``needs_input_grad`` has no entries for xa, xb, pool: with a block input
    # that wants no gradient the fp16 plan used to read needs[11] of that tuple (IndexError; fp32 never evaluated it)
    c = M.case("hs-32-32-no-x")
    ops.set_conv_dtype("f16")
    try:
        assert ops._block_bwd_plan(seen[c.id][0], R.needs_of(c)[:11], False, lambda: False) == nox
    finally:
        ops.set_conv_dtype(before)


# ------------------------------------------------------------------------------------------------------------------- 2. the model
@pytest.mark.parametrize("cid", ["tile-whole", "sign-16-32", "hs-pool-both", "hs-cat-64"])
def test_model_without_rounding_is_the_fp32_replay(cid):
    c = M.case(cid)
    ref = ref_of(c)
    own = M.step16(c, ref.t, ref.grads, ref.masks, M.Flags())
    r32 = R.step(c, ref.t, ref.grads, ref.masks, torch.float32)
    for k in names_of(c) + ["pre1", "pre2"]:
        assert torch.equal(own[k], r32[k]), k


def test_rounding_helpers():
    x = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 2.0 ** -25, 3 * 2.0 ** -25])
    assert M.half(x).tolist() == [1.0, 1.0 + 2.0 ** -9, 65504.0, 0.0, 2.0 ** -23]          # ties to even, subnormals, a tie at zero
    for m, s in ((1.0, 2.0 ** 13), (1.5, 2.0 ** 13), (2.0 - 2.0 ** -23, 2.0 ** 13), (2.0 ** -22, 2.0 ** 35), (3e-7, 2.0 ** 35), (0.0, 1.0)):
        got = M.grad_scale(torch.tensor([m, -m / 3]))
        assert got == s and (m == 0.0 or 2.0 ** 13 <= m * got < 2.0 ** 14), (m, got)
    assert M.grad_scale(torch.tensor([1e-7]), torch.tensor([-3.0])) == 2.0 ** 12             # one scale over two tensors: the larger rules


@pytest.mark.parametrize("cid", IDS)
def test_model_sits_at_fp16_rounding(cid):
    """d16 of every compared tensor: nowhere beyond 4e-3, and far above the fp32 replay's own 1e-6 on every tensor that fp16 rounding
    reaches in EVERY plan (conv2 has fp16 operands in all of them: out, the gradients behind conv2's data-gradient, w2 and g2; not
    b2 / bs, plain sums of the masked upstream gradient, and not ws / gs where the shortcut is a separate fp32 conv)"""
    c = M.case(cid)
    ref = ref_of(c)
    for k in names_of(c):
        d16 = R.rel_err(ref.r32[k].numpy(), ref.r64[k].numpy())
        print(f"{cid} {k}: d16 {d16:.3g}")
        assert d16 < 4e-3, (k, d16)
        if k in ("out", "pooled", "x", "xa", "xb", "w1", "g1", "b1", "w2", "g2"):
            assert d16 > 5e-5, (k, d16)


# ------------------------------------------------------------------------------------------------------------------- 3. the conditions
@pytest.mark.parametrize("cid", IDS)
def test_no_discrete_event_is_left_to_fp16_noise(cid):
    c = M.case(cid)
    ref = ref_of(c)
    i = ref.info
    noise = max(i["noise1"], i["noise2"])
    print(f"{cid}: min |pre| {i['margin']:.3g}  max |model pre - fp64 pre| {i['noise1']:.3g} / {i['noise2']:.3g}  margin / noise "
          f"{i['margin'] / noise:.3g}  pool gap {i['gap']:.3g}  zeroed windows {i['zeroed']:.3g}")
    assert 1e-4 < noise < 2e-2                           # the model does round (an fp32 replay sits at 1e-6)
    for v in list(ref.t.values()) + list(ref.grads.values()):          # every input is an fp32 value: the device gets the same numbers
        assert torch.equal(v, v.float().double()) and not v.requires_grad
    assert float(ref.grads["gout"].abs().max()) < 2e-6   # gradients at their real magnitude: fp16 subnormals without a scale
    if c.slope != 1.0:
        assert i["margin"] >= M.MARGIN_OVER_NOISE * noise
        for k in ("act1", "out"):
            assert 0.05 < float(ref.masks[k].double().mean()) < 0.95, k
    if c.pool:
        assert i["zeroed"] <= M.MAX_ZEROED_WINDOWS
        assert float(ref.grads["gpooled"].abs().max()) > 0
        # outside the windows taken out, the model pools the position the fp64 run pools
        at16 = torch.nn.functional.max_pool2d(ref.r32["out"], 2, return_indices=True)[1]
        at64 = torch.nn.functional.max_pool2d(ref.r64["out"], 2, return_indices=True)[1]
        assert torch.equal(at16 != at64, (at16 != at64) & (R.window_top2_gap(ref.r64["pre2"]) < i["gap"]))


# ------------------------------------------------------------------------------------------------------------------- 4. teeth
@pytest.mark.parametrize("cid", M.TEETH_CASES)
def test_model_passes_and_wrong_blocks_fail(cid):
    c = M.case(cid)
    ref = ref_of(c)
    names = names_of(c)
    assert R.compare(f"{cid} model", R.rows_of(c, ref.r32, ref, names), col="d16") == []
    for wrong in M.CORRUPTIONS:
        if wrong == "act1_bit" and c.slope == 1.0:       # (a mask bit means nothing at slope 1)
            continue
        got = M.corrupted(c, ref, wrong)
        fails = [f[0] for f in R.compare(f"{cid} {wrong}", R.rows_of(c, got, ref, names), col="d16")]
        assert fails, f"{wrong} passes the comparison: the bar or the norm is too weak"
        hit = {"act1_bit": "x", "stats2_row": "out", "dx_sc_image": "x", "w1_border_row": "w1", "g2_image": "g2", "noscale": "w2"}[wrong]
        assert hit in fails, (wrong, fails)
