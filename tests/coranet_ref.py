"""The CoraNet head arithmetic (reference trainer/coraNetTrainer.py:288-347, :168-208) restated in plain torch for arbitrary shapes
and dtypes -- the GPU tests evaluate it in fp64 as the reference of the fused kernels.  ``tests/test_coranet_cpu.py`` pins it to the
reference's own modules through ``tests/golden/coranet.npz``.  Also the shared description of that fixture's scenarios (seeds, shapes),
used by the generator, the CPU test and the GPU test.  Test infrastructure only: nothing here runs on the product path.

Logits are [N, 3L+1, H, W]: three (L+1)-class heads sharing the background logit (channel 0; head k owns channels 1+kL .. (k+1)L)."""
import numpy as np
import torch

from oracle import recipe

SMOOTH, EPS = 1e-5, 1e-8


def n_labels(z):
    c = z.shape[1]
    assert c >= 4 and (c - 1) % 3 == 0, c
    return (c - 1) // 3


def heads(z):
    """The three heads as separate [N, L+1, H, W] tensors (what the reference builds with torch.cat)."""
    L = n_labels(z)
    return [torch.cat([z[:, :1], z[:, 1 + k * L:1 + (k + 1) * L]], dim=1) for k in range(3)]


def soft_dice(x, y, batch_dice):
    """misc/loss.py:39-63: 1 - mean over the foreground classes of (2tp + s) / (2tp + fp + fn + s + 1e-8)."""
    p = torch.softmax(x, dim=1)
    hot = torch.zeros_like(p).scatter_(1, y.unsqueeze(1), 1.0)
    dims = (0, 2, 3) if batch_dice else (2, 3)
    tp, fp, fn = (p * hot).sum(dims), (p * (1 - hot)).sum(dims), ((1 - p) * hot).sum(dims)
    dc = (2 * tp + SMOOTH) / (2 * tp + fp + fn + SMOOTH + EPS)
    return 1.0 - (dc[1:] if batch_dice else dc[:, 1:]).mean()


def nll(x, y):
    """per-pixel -log softmax(x)[y], [N, H, W]"""
    return -torch.log_softmax(x, dim=1).gather(1, y.unsqueeze(1)).squeeze(1)


def weighted_ce(x, y, w):
    """nn.CrossEntropyLoss(weight=w), mean reduction: sum w[y] nll / sum w[y]"""
    wy = w.to(x.dtype)[y]
    return (wy * nll(x, y)).sum() / wy.sum()


def sup_loss(z, y, w_con, w_rad, weight_ce=0.5, weight_dc=0.5):
    """[S, dice+ce of head 0, con, rad] (:288-301)."""
    h0, h1, h2 = heads(z)
    cedc = weight_dc * soft_dice(h0, y, True) + weight_ce * nll(h0, y).mean()
    con, rad = weighted_ce(h1, y, w_con), weighted_ce(h2, y, w_rad)
    return torch.stack([(cedc + con + rad) / 4, cedc, con, rad])


def semi_loss(z, e, q, m, cw):
    """[certain, uncertain] (:304-341); ``e`` teacher logits, ``q`` pseudo labels, ``m`` 0/1 mask [N, H, W]."""
    m = m.to(z.dtype)
    hz, he = heads(z), heads(e.detach())
    certain = ((nll(hz[0], q) * m).sum() / (m.sum() + 1e-16) + soft_dice(hz[0], q, False)) / 2
    um = (1 - m).unsqueeze(1)
    unc = sum(cw * (((torch.softmax(a, 1) - torch.softmax(b, 1)) ** 2 * um).sum() / (um.sum() + 1e-16)) for a, b in zip(hz, he)) / 3
    return torch.stack([certain, unc])


def pseudo(z):
    """(argmax of head 0, (argmax of head 1 == argmax of head 2) as 0/1 float) (:189-208)."""
    h0, h1, h2 = heads(z)
    return torch.argmax(h0, 1), (torch.argmax(h1, 1) == torch.argmax(h2, 1)).to(torch.float32)


def ema(ema_params, params, alpha):
    """:168-174, out of place"""
    return [e * alpha + p * (1 - alpha) for e, p in zip(ema_params, params)]


def rampup(cur, length):
    ph = 1.0 - np.clip(cur, 0.0, length) / length
    return float(np.exp(-5.0 * ph * ph))


def binary_dc(a, b):
    a, b = np.asarray(a).astype(bool), np.asarray(b).astype(bool)
    den = np.count_nonzero(a) + np.count_nonzero(b)
    return 2.0 * np.count_nonzero(a & b) / float(den) if den else 0.0


# ---- the scenarios of tests/golden/coranet.npz (configuration of test_siblings_gpu.py: 3 classes, width 8, 64 x 64, bs 2, epoch 20)
L, WIDTH, SIZE, BS, EPOCH = 2, 8, 64, 2, 20
SEED_STUDENT, SEED_TEACHER = 301, 302
LR, MOMENTUM, WD, MAX_IT = 1e-2, 0.9, 1e-3, 200 * 150
W_CON, W_RAD = [1.0] + [5.0] * L, [5.0] + [1.0] * L
# name -> (first iteration, [seed of each consecutive step])
SCENARIOS = {"pre": (0, [310]), "t500": (500, [320]), "t1200": (1200, [330, 340])}
PRED_SEED, PRED_SLICES, VAL_SEED = 350, 4, 360


def shapes():
    return recipe.unet_shapes(1, 3 * L + 1, WIDTH)


def step_inputs(seed):
    """(labelled images, labels, unlabelled images) of one step"""
    return (recipe.synth_images((BS, 1, SIZE, SIZE), seed), recipe.synth_labels(BS, SIZE, SIZE, L + 1, seed + 1, block=8),
            recipe.synth_images((BS, 1, SIZE, SIZE), seed + 2))


def pred_inputs():
    return (recipe.synth_images((PRED_SLICES, 1, SIZE, SIZE), PRED_SEED),
            recipe.synth_labels(PRED_SLICES, SIZE, SIZE, L + 1, PRED_SEED + 1, block=8))


def val_inputs():
    return recipe.synth_images((BS, 1, SIZE, SIZE), VAL_SEED), recipe.synth_labels(BS, SIZE, SIZE, L + 1, VAL_SEED + 1, block=8)


def ema_alpha(it):
    return 0.0 if it < 100 else min(1 - 1 / (it + 1), 0.99)


def loss_case(seed=370, n=2, size=24):
    """Inputs of the loss-only case of the fixture: logits 2 * randn of student and teacher, labels, pseudo labels, mask."""
    rs = np.random.RandomState(seed)
    z = torch.from_numpy(2 * rs.standard_normal((n, 3 * L + 1, size, size))).float()
    e = torch.from_numpy(2 * rs.standard_normal((n, 3 * L + 1, size, size))).float()
    y = torch.from_numpy(rs.randint(0, L + 1, (n, size, size)).astype(np.int64))
    q = torch.from_numpy(rs.randint(0, L + 1, (n, size, size)).astype(np.int64))
    m = torch.from_numpy((rs.uniform(size=(n, size, size)) < 0.6).astype(np.float32))
    return z, e, y, q, m
