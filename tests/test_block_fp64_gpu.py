"""The fused BasicBlock (``ops.BasicBlockFn``: forward and its hand-written backward, as ``basic_block``, ``basic_block_cat`` and
``basic_block_pool`` launch it) end to end against fp64, on every branch of its plan, with no LeakyReLU sign and no pooling argmax
left to rounding.

The kernels behind the plan are each held to fp64 at the C ABI (test_conv3x3_edges_gpu, test_conv_families_gpu, test_instnorm_gpu,
test_restail_gpu); this file holds their COMPOSITION to it: which statistics feed which stage, which operands a weight gradient reads,
where the shortcut's gradient is added, what comes back for which ``needs_input_grad``.  tests/block_ref.py makes the inputs (the two
InstanceNorm shifts placed so that no pre-activation is within MARGIN of zero; near-tie pooling windows get no pooled gradient), the
fp64 reference and the fp32 CPU replay of it; tests/test_block_ref_cpu.py pins all three, the cases' plans included, without a device.

Per case: the launches are the ones the plan names, in order (``block_ref.expected_launches``); the sign pattern of ``out`` is the
reference's, exactly, and ``pooled`` is the window maximum of the device's own ``out``, exactly; ``out``, ``pooled`` and every
gradient meet max(4 d32, floor) on max |got - fp64| / max |fp64| (``block_ref.compare``: no quantile, no l2 bar); gradients that were
not asked for are None; a second run gives the same bits and leaves the tickets zeroed.

A pool block takes the routed backward ``smsut_restail_bwd_pool`` when both outputs bring a gradient.  With the pooled path's alone
``smsut_maxpool2_bwd`` makes the tail's upstream gradient first, with the skip's alone the backward is the plain block's: an output
without a gradient reaches ``BasicBlockFn.backward`` as None.  (It used to arrive as a materialised NCHW tensor of zeros, which was
converted by a layout copy and routed; pool-only-pooled / pool-only-skip found that through ``ops.layout_copies()``.)

Measured on an MI355X: see DESIGN.md 4b (worst err / bar per case)."""
import pytest
import torch
import torch.nn.functional as F

import block_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    assert ops.IN_EPS == R.IN_EPS
    prev = ops.conv_dtype()
    ops.set_conv_dtype("f32")
    yield ops
    ops.set_conv_dtype(prev)


def act_dev(t):
    return t.float().cuda().contiguous(memory_format=torch.channels_last)


def w_dev(ops, w):
    out = ops.new_weight(*w.shape, device="cuda")
    out.copy_(w.float())
    return out


def run(ops, c, ref):
    """one forward + backward on the device -> (results by name on the CPU: out, pooled, gradients (None where none came back);
    entry points launched by the block, in order)"""
    from smsut_amd import profiling
    t = ref.t
    frozen = ("w1", "ws") if c.needs == "frozen" else ()
    P = {k: (w_dev(ops, t[k]) if t[k].dim() == 4 else t[k].float().cuda()).requires_grad_(k not in frozen) for k in R.PARAMS if k in t}
    X = {k: act_dev(t[k]).requires_grad_(c.needs != "no_x") for k in ("x", "xa", "xb") if k in t}
    prm = [P.get(k) for k in R.PARAMS]
    if c.form == "catmat":
        x = ops.concat_channels(X["xa"], X["xb"])        # (its own node, outside the record: the block bypasses it)
        assert getattr(x, "_smsut_cat_parts", None) is not None
    elif c.form == "cat":
        x = ops.concat_channels_deferred(X["xa"], X["xb"])
        assert isinstance(x, ops.CatParts) and ops.basic_block_cat_fusable(x, P["w1"], P["ws"])
    else:
        x = X["x"]
        assert ops.basic_block_fusable(x, P["w1"], P.get("ws"))
    gout = act_dev(ref.grads["gout"])
    gpooled = act_dev(ref.grads["gpooled"]) if c.pool else None
    box = {}

    def step():
        if c.pool:
            assert ops.basic_block_pool_fusable(x, P["w1"], P["ws"])
            out, pooled = ops.basic_block_pool(x, *prm, c.slope)
            outs, gs = {"both": ([out, pooled], [gout, gpooled]), "pooled": ([pooled], [gpooled]), "skip": ([out], [gout])}[c.grads]
        else:
            out, pooled = (ops.basic_block_cat if c.form == "cat" else ops.basic_block)(x, *prm, c.slope), None
            outs, gs = [out], [gout]
        box.update(out=out.detach(), pooled=None if pooled is None else pooled.detach())
        torch.autograd.backward(outs, gs)

    copies = ops.layout_copies()
    rec = profiling.record_step(step)
    assert ops.layout_copies() == copies
    got = {k: None if v is None else v.cpu() for k, v in box.items()}
    for k, v in {**X, **P}.items():
        got[k] = None if v.grad is None else v.grad.cpu()
    return got, [name for name, _ in rec]


@pytest.mark.parametrize("cid", [c.id for c in R.CASES])
def test_fused_block_vs_fp64(ops, cid):
    if not ops.FUSED_BLOCK:
        pytest.skip("SMSUT_FUSED_BLOCK=0 in the environment")
    from smsut_amd import _hip as H
    c = R.case(cid)
    ref = R.reference(c)
    p, b = R.plans(ops, c, torch.empty(R.like_shape(c), device="cuda"), fin=ops._fin_available(torch.empty(1, device="cuda")))
    fwd, bwd = R.expected_launches(H, p, b, c.pool and c.grads == "pooled")
    print(f"{cid}: {p}\n{cid}: {b}")
    got, names = run(ops, c, ref)
    got2, names2 = run(ops, c, ref)
    print(f"{cid}: " + " ".join(k.replace("smsut_", "") for k in names))
    wanted = [k for k in R.grad_names(c) if not (c.needs == "no_x" and k in ("x", "xa", "xb")) and not (c.needs == "frozen" and k in ("w1", "ws"))]
    for k in ("x", "xa", "xb") + R.PARAMS:               # what was not asked for does not come back
        assert (got.get(k) is not None) == (k in wanted), k
    names_cmp = ["out"] + (["pooled"] if c.pool else []) + wanted
    fails = R.compare(cid, R.rows_of(c, got, ref, names_cmp))        # (prints every figure; asserted below)

    # the launches the plan names, in order
    assert names == fwd + bwd, (names, fwd + bwd)
    if c.needs == "no_x":                                # nothing computes a block-input gradient
        assert b.dx is None and not [k for k in names if k in ("smsut_conv2d_dgrad_mfma_sc", "smsut_conv1x1_fwd_split", "smsut_concat2")]
        assert names.count("smsut_conv2d_fwd_mfma") == (0 if b.pers2 else 1) and names.count("smsut_conv1x1_fwd") == fwd.count("smsut_conv1x1_fwd")
    # discrete events: exactly the reference's
    assert torch.equal(got["out"] > 0, ref.masks["out"]), "a sign of out differs from the fp64 run's"
    if c.pool:
        assert torch.equal(got["pooled"], F.max_pool2d(got["out"], 2)), "pooled is not the window maximum of the device's own out"
    # values
    assert not fails, (cid, fails)
    # the second run: the same launches, the same bits (tickets and workspaces leave nothing behind)
    assert names2 == names
    for k in names_cmp:
        assert torch.equal(got2[k], got[k]), k
    ring = ops._TICKET_RING.get(0)
    if ring is not None:
        assert int(ring[0].abs().sum()) == 0, "a launch left tickets behind"
