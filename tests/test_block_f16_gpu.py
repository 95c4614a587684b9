"""The fused BasicBlock with fp16 operands and half storage (``ops.set_conv_dtype("f16")``) end to end against fp64, on
every branch of its fp16 plan: ``f16a`` / ``f16`` per conv, ``hs``, the 8 -> 16 first block, the tail forms "hs" / "amax" / "pool",
the fused-shortcut gradient kernels and their ONE scale, the amax hand-over slots, the fp32 weight-gradient fallback.

The fp16 kernels are pinned one by one, exactly, by test_f16_edges_gpu.py; test_f16_gpu.py holds the block to the fp32 GPU path at
flip-dominated l2 bars.  This file holds the COMPOSITION to an independent reference at what fp16 rounding itself allows: the reference
is ``block_ref.step(..., torch.float64)``; the yardstick d16 is the CPU rounding model of tests/block_f16_ref.py (fp16 roundings where
the plan puts them, nowhere else); every tensor meets max(4 d16, floor) on max |got - fp64| / max |fp64| -- bars of 2e-4 .. 7e-3 that
a scale taken from the wrong slots (a wrong power of two: lost bits or a flush to zero) or a statistics set fed to the wrong stage
(1e-2) cannot pass.  No sign and no argmax is left to fp16 noise: smooth cases run at slope 1.0 (same kernels, same plan), sign cases
at slope 0.01 on planes where the placed shifts keep every pre-activation 6 x the model's noise from zero
(tests/test_block_f16_ref_cpu.py asserts the conditions, the plans and that wrong blocks miss these bars).

Per case: the plan fields of the branch it claims; the launches the plan names, in order, the scale launches among them; no layout
copy; values below their bars; None for what was not asked for; ``pooled`` the window maximum of the device's own ``out``; for sign
cases the sign pattern of ``out`` the reference's, exactly; a second run with the same bits and the tickets zeroed; on one case
``out`` differs from the fp32 mode's.  The upstream gradients are 2^-22 of block_ref's: unscaled, they underflow in fp16.

Measured on an MI355X: see DESIGN.md 4b (worst err / bar per case)."""
import pytest
import torch
import torch.nn.functional as F

import block_f16_ref as M
import block_ref as R
from test_block_fp64_gpu import run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    assert ops.IN_EPS == R.IN_EPS
    prev = ops.conv_dtype()
    ops.set_conv_dtype("f16")
    yield ops
    ops.set_conv_dtype(prev)


@pytest.mark.parametrize("cid", [c.id for c in M.F16_CASES])
def test_fused_f16_block_vs_fp64(ops, cid):
    if not ops.FUSED_BLOCK:
        pytest.skip("SMSUT_FUSED_BLOCK=0 in the environment")
    from smsut_amd import _hip as H
    assert ops.conv_dtype() == "f16" and ops.AMAX_HANDOVER
    c = M.case(cid)
    p, b = R.plans(ops, c, torch.empty(R.like_shape(c), device="cuda"), fin=ops._fin_available(torch.empty(1, device="cuda")))
    assert (p, b) == M.plans_cpu(c, ops)                    # the plan the CPU pins, the model's flags were read from
    M.check_plan(c, p, b)
    ref = M.reference(c, M.flags_of(p, b))
    fwd, bwd = R.expected_launches(H, p, b, c.pool and c.grads == "pooled")
    print(f"{cid}: {p}\n{cid}: {b}")
    got, names = run(ops, c, ref)
    got2, names2 = run(ops, c, ref)
    print(f"{cid}: " + " ".join(k.replace("smsut_", "") for k in names))
    wanted = [k for k in R.grad_names(c) if not (c.needs == "no_x" and k in ("x", "xa", "xb")) and not (c.needs == "frozen" and k in ("w1", "ws"))]
    for k in ("x", "xa", "xb") + R.PARAMS:               # what was not asked for does not come back
        assert (got.get(k) is not None) == (k in wanted), k
    names_cmp = ["out"] + (["pooled"] if c.pool else []) + wanted
    fails = R.compare(cid, R.rows_of(c, got, ref, names_cmp), col="d16")       # (prints every figure; asserted below)

    # the launches the plan names, in order: the fp16 kernels, and the launches that make the gradient operands' scales
    assert names == fwd + bwd, (names, fwd + bwd)
    scales = [k for k in names if k.startswith("smsut_absmax_")]
    assert len(scales) == 1 + int(p.f16a) and scales[0] == "smsut_absmax_finish", scales      # gy2's always comes from the tail's slots
    if p.f16a:                                           # gy1's (or [gy1 | gs_t]'s) from its producer's slots on the persistent path, else by a pass
        assert scales[1] == ("smsut_absmax_finish" if b.pers2 else "smsut_absmax_scale2" if b.fused_wsc16 or b.fused_dsc16 else "smsut_absmax_scale"), scales
    if c.needs == "no_x":
        assert b.dx is None and not [k for k in names if "dgrad_mfma_sc" in k or k in ("smsut_conv1x1_fwd_split", "smsut_concat2", "smsut_conv1x1_fwd")]
    # discrete events: exactly the reference's
    if c.slope != 1.0:
        assert torch.equal(got["out"] > 0, ref.masks["out"]), "a sign of out differs from the fp64 run's"
    if c.pool:
        assert torch.equal(got["pooled"], F.max_pool2d(got["out"], 2)), "pooled is not the window maximum of the device's own out"
    # values
    for k in names_cmp:
        assert bool(torch.isfinite(got[k]).all()), k
    assert not fails, (cid, fails)
    # the second run: the same launches, the same bits (tickets and workspaces leave nothing behind)
    assert names2 == names
    for k in names_cmp:
        assert torch.equal(got2[k], got[k]), k
    ring = ops._TICKET_RING.get(0)
    if ring is not None:
        assert int(ring[0].abs().sum()) == 0, "a launch left tickets behind"
    if cid == M.FP32_TWIN_CASE:                          # the fp16 kernels really ran: the fp32 mode gives other bits, closer to fp64
        ops.set_conv_dtype("f32")
        try:
            got32, names32 = run(ops, c, ref)
        finally:
            ops.set_conv_dtype("f16")
        assert not [k for k in names32 if "f16" in k or "_hs" in k or "absmax" in k], names32
        assert not torch.equal(got32["out"], got["out"])
        e32, e16 = (R.rel_err(g["out"].numpy(), ref.r64["out"].numpy()) for g in (got32, got))
        print(f"{cid}: out vs fp64: fp32 mode {e32:.3g}, fp16 mode {e16:.3g}")
        assert e32 < R.FLOORS["fwd"] < e16
