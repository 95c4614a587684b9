"""fp64 reference of the discriminator's WGAN-GP pass (tests/test_gp_pass_gpu.py; pinned to torch autograd of the ordinary ``F.leaky_relu``
composition by tests/test_gp_ref_cpu.py): a stride-2 ``BottleBlock`` in both of its forms, the ``Discriminator`` built from them, and the
step that differentiates them twice, restated in functional torch on the CPU.  Tensors are logical NCHW / OIHW; parameters are dicts with
the modules' ``state_dict`` keys.

Every LeakyReLU is ``z * where(mask, 1, slope)`` with a GIVEN boolean mask.  With the mask fixed the function is smooth, so a run in
fp32 and one in fp64 differ by rounding only, and a pre-activation within an ulp of zero cannot flip between the GPU and the reference and
move a 3x3 patch of gradients by O(1e-3).  ``masks`` maps a site to its mask ("bn1" and "out" of a block; "main.1" (the stem's
activation), "main.<i>.bn1" and "main.<i>" in the discriminator); a site that is missing is filled in from the run's own pre-activation,
which is how the CPU test gets the ordinary LeakyReLU."""
import torch
import torch.nn.functional as F

IN_EPS = 1e-5                # == ops.IN_EPS (asserted by the GPU test)
SLOPE = 1e-2                 # blocks.LRELU_SLOPE and nn.LeakyReLU()'s default: every activation of the discriminator

# (n, ci, co, h): stride-2 BottleBlocks.  ci != co: the downsample form (1x1 conv + IN on avg_pool2(x)); ci == co: the identity form
# (shortcut = avg_pool2(x)); the last one has the channels and the plane of the production discriminator's capped block (8x8 -> 4x4)
BLOCK_CASES = [(2, 16, 32, 16), (3, 8, 16, 32), (2, 32, 32, 8), (2, 256, 256, 8)]
DISC = dict(size=32, n_modal=4, width=8, max_width=16, batch=3)      # stem 1->8, 8->16 (downsample), 16->16 (identity), k = 4 head
SINGLE_OP_BARS = {"out": 1e-5, "dydx": 1e-5, "second": 5e-5, "wgrad": 5e-5}
# kernels between input and output: conv1, IN + act, pool, conv2, IN, pool, (1x1 conv, IN,) add + act
BLOCK_OPS = {True: 9, False: 7}


def act(z, masks, key, slope):
    m = masks.get(key)
    if m is None:
        m = masks[key] = z.detach() > 0
    assert m.dtype == torch.bool and m.shape == z.shape, key
    return z * torch.where(m, torch.ones((), dtype=z.dtype), torch.full((), slope, dtype=z.dtype))


def inorm(x, p, pre):
    return F.instance_norm(x, weight=p[pre + "weight"], bias=p[pre + "bias"], eps=IN_EPS)


def bottle_block(x, p, slope, stride, masks, pre=""):
    """blocks.BottleBlock.forward with instance norm.  The form follows the parameters: with ``downsample.0.weight`` the shortcut is
    IN(conv1x1(avg_pool2(x))), without it avg_pool2(x) (stride 2) or x."""
    idn = F.avg_pool2d(x, 2) if stride == 2 else x
    y = act(inorm(F.conv2d(x, p[pre + "conv1.weight"], padding=1), p, pre + "bn1."), masks, pre + "bn1", slope)
    if stride == 2:
        y = F.avg_pool2d(y, 2)
    y = inorm(F.conv2d(y, p[pre + "conv2.weight"], padding=1), p, pre + "bn2.")
    if pre + "downsample.0.weight" in p:
        idn = inorm(F.conv2d(idn, p[pre + "downsample.0.weight"]), p, pre + "downsample.1.")
    return act(y + idn, masks, (pre[:-1] if pre else "out"), slope)


def discriminator(x, p, masks):
    """ugan.Discriminator.forward: (out_src [n,1,h,w], out_cls [n, n_modal])"""
    h = act(F.conv2d(x, p["main.0.weight"], p["main.0.bias"], stride=2, padding=1), masks, "main.1", SLOPE)
    i = 2
    while f"main.{i}.conv1.weight" in p:
        h = bottle_block(h, p, SLOPE, 2, masks, pre=f"main.{i}.")
        i += 1
    cls = F.conv2d(h, p["conv_cls.weight"])
    assert cls.shape[2:] == (1, 1), "conv_cls is a full-window conv"
    return F.conv2d(h, p["conv_src.weight"], padding=1), cls.reshape(cls.shape[0], cls.shape[1])


def disc_ops(p):
    """kernels between input and out_src: stem conv, activation, the blocks, conv_src"""
    n, i = 3, 2
    while f"main.{i}.conv1.weight" in p:
        n += BLOCK_OPS[f"main.{i}.downsample.0.weight" in p]
        i += 1
    return n


def gp_step(fwd, x_hat, params, a, b, extra=None, cot=None, dtype=torch.float64):
    """The gradient-penalty step on ``src, more = fwd(x_hat, params)``:
        dydx = grad(src, x_hat, ones, create_graph=True);  gp = mean((||dydx||_2 per sample - 1)^2);
        loss = a * src.mean() + b * gp (+ extra(params) -> (its loss, its outputs));  the backward of loss, through dydx again.
    ``cot`` replaces the ones by a cotangent that is differentiated too ("d_cot"): what a block inside the discriminator passes on to
    the layer after it, and the only consumer of the final activation's second-order result.
    Returns {"src", "more", "dydx", "gp", "loss", "d_x_hat", "d_cot", "grads": {name: d loss / d parameter}, + extra's outputs}, detached."""
    x = x_hat.detach().to(dtype).requires_grad_(True)
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    src, more = fwd(x, p)
    c = torch.ones_like(src) if cot is None else cot.detach().to(dtype).requires_grad_(True)
    (dydx,) = torch.autograd.grad(src, x, c, create_graph=True)
    gp = ((dydx.flatten(1).square().sum(1).sqrt() - 1.0) ** 2).mean()
    loss = a * src.mean() + b * gp
    out = {}
    if extra is not None:
        more_loss, out = extra(p, dtype)
        loss = loss + more_loss
    grads = torch.autograd.grad(loss, [x] + list(p.values()) + ([c] if cot is not None else []), allow_unused=True)
    out = {k: v.detach() for k, v in out.items()}
    out.update(src=src.detach(), more=None if more is None else more.detach(), dydx=dydx.detach(), gp=gp.detach(), loss=loss.detach(),
               d_x_hat=grads[0], d_cot=grads[-1] if cot is not None else None, grads=dict(zip(p, grads[1:])))
    return out


def replay(dtype, *args, **kwargs):
    """the same restatement in fp32 or fp64: the distance between the two is the rounding noise of this arithmetic at these shapes"""
    return gp_step(*args, dtype=dtype, **kwargs)


def block_step(x_hat, params, masks, a, b, cot=None, dtype=torch.float64):
    return gp_step(lambda x, p: (bottle_block(x, p, SLOPE, 2, masks), None), x_hat, params, a, b, cot=cot, dtype=dtype)


def disc_step(x, xf, x_hat, tgt, params, masks_rf, masks_hat, lambda_cls=1.0, lambda_gp=10.0, dtype=torch.float64):
    """The trainers' D step (uganTrainer.train_step): D on cat([x, xf]) gives d_real = -mean(src[:b]), d_fake = mean(src[b:]) and
    d_cls = cross_entropy(cls[:b], tgt); D on x_hat gives the penalty; loss = d_real + d_fake + lambda_cls d_cls + lambda_gp gp."""
    b = x.shape[0]

    def real_fake(p, dt):
        src, cls = discriminator(torch.cat([x, xf], 0).to(dt), p, masks_rf)
        d_real, d_fake, d_cls = -src[:b].mean(), src[b:].mean(), F.cross_entropy(cls[:b], tgt)
        return d_real + d_fake + lambda_cls * d_cls, dict(src_rf=src, cls_rf=cls, d_real=d_real, d_fake=d_fake, d_cls=d_cls)

    return gp_step(lambda xh, p: discriminator(xh, p, masks_hat), x_hat, params, 0.0, lambda_gp, extra=real_fake, dtype=dtype)


# ---- seeded parameters and inputs of the CPU test (the GPU test takes them from its modules) --------------------------------------
def _rn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def block_params(ci, co, seed):
    """conv weights ~ N(0, 1 / fan_in) + 0.1 N(0, 1), gamma ~ 1 + 0.1 N, beta ~ 0.1 N -- the spread the GPU test's nudged modules have"""
    g = torch.Generator().manual_seed(seed)
    p = {"conv1.weight": _rn(g, co, ci, 3, 3) / (9 * ci) ** 0.5 + 0.1 * _rn(g, co, ci, 3, 3),
         "bn1.weight": 1 + 0.1 * _rn(g, co), "bn1.bias": 0.1 * _rn(g, co),
         "conv2.weight": _rn(g, co, co, 3, 3) / (9 * co) ** 0.5 + 0.1 * _rn(g, co, co, 3, 3),
         "bn2.weight": 1 + 0.1 * _rn(g, co), "bn2.bias": 0.1 * _rn(g, co)}
    if ci != co:
        p.update({"downsample.0.weight": _rn(g, co, ci, 1, 1) / ci ** 0.5 + 0.1 * _rn(g, co, ci, 1, 1),
                  "downsample.1.weight": 1 + 0.1 * _rn(g, co), "downsample.1.bias": 0.1 * _rn(g, co)})
    return p


def block_input(n, ci, h, seed):
    return _rn(torch.Generator().manual_seed(seed), n, ci, h, h)


def disc_inputs(seed, size=DISC["size"], batch=DISC["batch"], n_modal=DISC["n_modal"]):
    """(x, xf, alpha [b,1,1,1], tgt [b]): images in the range the trainers feed (clamp(0.5 N, -1, 1)), alpha ~ N(0, 1) as the trainers draw it"""
    g = torch.Generator().manual_seed(seed)
    x = (0.5 * _rn(g, batch, 1, size, size)).clamp(-1, 1).float()
    xf = (0.5 * _rn(g, batch, 1, size, size)).clamp(-1, 1).float()
    alpha = _rn(g, batch, 1, 1, 1).float()
    tgt = torch.randint(0, n_modal, (batch,), generator=g)
    return x, xf, alpha, tgt
