#!/usr/bin/env python3
"""Generator of tests/golden/uamt.npz: the reference's ``network.unet.UNet`` and ``misc.loss`` on the CPU, with the uncertainty-aware
mean teacher's training arithmetic (UA-MT: ``meanTeacherTrainer``'s iteration with the published uncertainty mask on its consistency
term; the trainer for it is not in the tree yet) replayed with torch CPU ops around them.  Run on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_uamt_golden.py

Same method as make_dtc_golden.py.  Scenario, seeds, shapes and the fixed noises come from tests/uamt_ref.py; student and teacher are
filled by ``oracle.recipe.fill`` from different seeds.  Two steps at iterations 300 and 301 (consistency on, EMA alpha 0.99), 2 + 2
slices of 32 x 32, base width 8, C = 5, ``mc_samples`` 4 in passes of 2, epoch 20 (ramp-up weight exp(-5/9) = 0.574).

``threshold_max``.  A randomly initialised teacher is unconfident: at ln 2 the mask of this scenario would be nearly empty.  The
generator therefore chooses ``threshold_max``: among the mid-points of the widest gaps between neighbouring fp64 uncertainties of the
first step whose kept share lies in [0.4, 0.6], the one whose smallest distance |H - thr| over BOTH steps of the fp64 replay is
largest.  It asserts that ``kept`` lies in [0.3, 0.7] on both steps and that the fp32 and the fp64 replay agree on every mask bit, and
records the value (a GPU test of the trainer sets its ``threshold_max`` from the fixture).

Recorded (arrays and key names only):
  * ``threshold_max``, ``thr`` [2] (the two steps' thresholds), ``gap`` (the smallest |H - thr| of the fp64 replay over both steps);
  * ``scalars32`` / ``scalars64`` [2, 4] = [seg, L, kept, meanH] of the two steps in fp32 / fp64;
  * ``post32_*`` / ``post64_*``: decoder.fc.weight, decoder.layer1.conv2.weight, encoder.pre_conv.weight of the student after the second
    step, ``ema32_fc``: the teacher's decoder.fc.weight;
  * ``mask0`` (uint8, packed bits) and ``unc0`` (fp64 rounded once to fp32) of the first step;
  * ``head{i}_out`` / ``head{i}_mask``: ``uamt_ref.loss_ref`` on the small head cases ``uamt_ref.HEAD_CASES`` at thr = 0.75 ln 2.

Figures this generator measured and printed, and the bars they give a GPU test of the trainer:
    fp32 vs fp64 replay, second-step scalars: max relative distance 7.1e-08   -> bar max(4 x, 2e-2) = 2e-2
    weights after it:                         max rel_err           6.6e-08   -> bar max(4 x, 2e-3) = 2e-3 (the mean teacher's floor)
    threshold_max 1.92023, thresholds 1.443743 / 1.443744; kept 0.5791 / 0.5566; smallest |H - thr| 4.3e-04
The bar on the weights is as wide as what two steps change (the update is 2.3e-3 / 1.3e-3 / 3.5e-3 of the three tensors), so such a
test also compares the UPDATE: rel_err(w_after - w_init, post32 - w_init) per tensor for fc / layer1.conv2 / pre_conv, bar 0.02.
fp32 CPU replays of a wrong trainer against the committed ``post32_*``:
    the fp64 replay (the size of rounding):        2.9e-05 / 4.3e-05 / 1.6e-05   -> passes
    lr = 0 (no backward or no optimizer step):     1.0     / 1.0     / 1.0       -> fails on all three
    lambda_semi = 0 (consistency term dropped):    0.24    / 0.13    / 0.21      -> fails on all three
    thr = +inf (the mask ignored):                 0.069   / 0.042   / 0.083     -> fails on all three
0.02 is more than four hundred times the fp32 / fp64 distance of the update and less than half the smallest figure a wrong trainer
gives."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SMSUT_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from network.unet import UNet                      # noqa: E402  (reference)
from misc.loss import DiceAndCrossEntropyLoss      # noqa: E402  (reference)

import uamt_ref as R                               # noqa: E402  (ours)
from oracle import recipe                          # noqa: E402  (ours)

torch.set_num_threads(8)


def npy(t):
    return t.detach().cpu().numpy().copy()


def fresh(seed, dtype):
    net = UNet(1, R.C, R.WIDTH, "instance", "lrelu")
    shapes = R.shapes()
    sd_ref = net.state_dict()
    assert list(sd_ref.keys()) == list(shapes.keys())
    for k, v in sd_ref.items():
        assert tuple(v.shape) == tuple(shapes[k]), (k, tuple(v.shape), shapes[k])
    net.load_state_dict(recipe.fill(shapes, seed))
    return net.to(dtype).train()


def replay(dtype, threshold_max, lr=R.LR, lambda_semi=R.LAMBDA_SEMI, use_mask=True):
    """-> scalars [2, 4], student weights after the second step, teacher fc, per step (H fp64 [BS, S, S], mask bool, thr)"""
    stu, ema = fresh(R.SEED_NET, dtype), fresh(R.SEED_EMA, dtype)
    for p in ema.parameters():
        p.detach_()
    crit = DiceAndCrossEntropyLoss(0.5, 0.5, batch_dice=True)
    opt = torch.optim.SGD(stu.parameters(), lr=lr, momentum=R.MOMENTUM, weight_decay=R.WD)
    weight = lambda_semi * R.rampup(R.EPOCH, R.RAMPUP)
    scal, maps = [], []
    for k, seed in enumerate(R.STEP_SEEDS):
        it = R.IT0 + k
        img, msk, noise, mc_noise = (t if t.dtype == torch.int64 else t.to(dtype) for t in R.step_inputs(seed))
        ul = img[R.BS:]
        out = stu(img)
        with torch.no_grad():
            ema_out = ema(ul + noise)
            # the published composition: T stochastic passes in chunks, softmax, reshape to [T, N, ...], mean, entropy
            preds = torch.cat([ema(ul.repeat(R.MC_CHUNK, 1, 1, 1) + mc_noise[t0 * R.BS:(t0 + R.MC_CHUNK) * R.BS])
                               for t0 in range(0, R.MC_SAMPLES, R.MC_CHUNK)])
            preds = torch.softmax(preds, dim=1).reshape(R.MC_SAMPLES, R.BS, R.C, R.SIZE, R.SIZE).mean(dim=0)
            unc = -1.0 * torch.sum(preds * torch.log(preds + 1e-6), dim=1, keepdim=True)
        thr = R.threshold(it, R.MAX_IT, threshold_max) if use_mask else float("inf")
        mask = (unc < thr).to(dtype)
        dist = (torch.softmax(out[R.BS:], dim=1) - torch.softmax(ema_out, dim=1)) ** 2
        semi = torch.sum(mask * dist) / (2 * torch.sum(mask) + 1e-16)
        seg = crit(out[:R.BS], msk)
        total = seg + weight * semi
        opt.zero_grad(); total.backward(); opt.step()
        alpha = min(1 - 1 / (it + 1), R.EMA_DECAY)
        for ep, p_ in zip(ema.parameters(), stu.parameters()):
            ep.data.mul_(alpha).add_(p_.data, alpha=1 - alpha)
        for g in opt.param_groups:
            g["lr"] = lr * (1.0 - it / R.MAX_IT) ** 0.9
        scal.append([seg.item(), semi.item(), mask.mean().item(), unc.mean().item()])
        maps.append((npy(unc[:, 0]).astype(np.float64), npy(mask[:, 0]) > 0, thr))
    sd = stu.state_dict()
    return (np.array(scal, dtype=np.float64), {k: npy(sd[v]).astype(np.float64) for k, v in R.POST.items()},
            npy(ema.state_dict()["decoder.fc.weight"]), maps)


def choose_threshold_max():
    """see the module docstring"""
    h0 = np.sort(replay(torch.float64, 1e9)[3][0][0].ravel())
    n = h0.size
    lo, hi = int(0.4 * n), int(0.6 * n)
    gaps = h0[lo + 1:hi + 1] - h0[lo:hi]
    scale = R.threshold(R.IT0, R.MAX_IT, 1.0)
    best = None
    for j in np.argsort(gaps)[::-1][:40]:
        cand = float(np.float32(0.5 * (h0[lo + j] + h0[lo + j + 1]) / scale))
        maps = replay(torch.float64, cand)[3]
        gap = min(float(np.abs(h - thr).min()) for h, _, thr in maps)
        if best is None or gap > best[1]:
            best = (cand, gap)
    return best


def main():
    threshold_max, gap = choose_threshold_max()
    rec = dict(C=R.C, width=R.WIDTH, H=R.SIZE, bs=R.BS, epoch=R.EPOCH, it0=R.IT0, threshold_max=np.float64(threshold_max), gap=np.float64(gap))
    s32, p32, e32, m32 = replay(torch.float32, threshold_max)
    s64, p64, _, m64 = replay(torch.float64, threshold_max)
    for k in range(2):
        assert 0.3 <= s64[k, 2] <= 0.7 and 0.3 <= s32[k, 2] <= 0.7, (s32, s64)
        assert np.array_equal(m32[k][1], m64[k][1]), "fp32 and fp64 replays disagree on a mask bit"
    rec["thr"] = np.array([m[2] for m in m64], dtype=np.float64)
    rec["scalars32"], rec["scalars64"] = s32, s64
    for k in R.POST:
        rec["post32_" + k], rec["post64_" + k] = p32[k].astype(np.float32), p64[k]
    rec["ema32_fc"] = e32.astype(np.float32)
    rec["mask0"] = np.packbits(m64[0][1].ravel())
    rec["unc0"] = m64[0][0].astype(np.float32)
    for i, shp in enumerate(R.HEAD_CASES):
        z, e, u = R.case(*shp)
        out, mask, _ = R.loss_ref(z, e, u, R.THRESHOLDS[0])
        rec[f"head{i}_out"], rec[f"head{i}_mask"] = npy(out), npy(mask).astype(np.uint8)

    d_scal = float((np.abs(s32[1] - s64[1]) / np.abs(s64[1])).max())
    d_w = max(float(np.abs(p32[k] - p64[k]).max() / np.abs(p64[k]).max()) for k in R.POST)
    print("fp32 vs fp64 replay: first-step scalars rel %.1e, second-step scalars rel %.1e, weights rel_err %.1e"
          % (float((np.abs(s32[0] - s64[0]) / np.abs(s64[0])).max()), d_scal, d_w))
    print("bars of the GPU test: scalars %.1e, weights %.1e" % (max(4 * d_scal, 2e-2), max(4 * d_w, 2e-3)))
    print("threshold_max %.6g, thresholds %s, kept %s, smallest |H - thr| %.1e" % (threshold_max, rec["thr"], s64[:, 2], gap))

    init = {k: recipe.fill(R.shapes(), R.SEED_NET)[v].numpy().astype(np.float64) for k, v in R.POST.items()}
    upd = lambda p: {k: float(np.abs((p[k] - init[k]) - (p32[k] - init[k])).max() / np.abs(p32[k] - init[k]).max()) for k in R.POST}
    print("update rel_err of the fp64 replay:", upd(p64))
    for name, kw in (("lr = 0", dict(lr=0.0)), ("lambda_semi = 0", dict(lambda_semi=0.0)), ("thr = +inf", dict(use_mask=False))):
        print("update rel_err with %s:" % name, upd(replay(torch.float32, threshold_max, **kw)[1]))
    print("size of the update, rel_err(post32, init):", {k: float(np.abs(p32[k] - init[k]).max() / np.abs(init[k]).max()) for k in R.POST})

    path = os.path.join(HERE, "uamt.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")
    print("scalars32", s32, "\nscalars64", s64)


if __name__ == "__main__":
    main()
