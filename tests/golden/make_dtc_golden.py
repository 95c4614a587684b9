#!/usr/bin/env python3
"""Generator of tests/golden/dtc.npz: the reference's ``network.dtc.UNet`` (with its ``network.blocks`` and ``misc.loss`` modules) on
the CPU, the dual-task-consistency training arithmetic replayed with torch CPU ops around it, and signed distance maps from
``scipy.ndimage.distance_transform_edt``.  Run on the CPU:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dtc_golden.py

Same method as make_coranet_golden.py.  The reference ships the network without a trainer; the replayed iteration is the one
``trainer/dtcTrainer.py`` documents (DiceCE on the labelled logits + beta * MSE(tanh head, sdf) + consistency * rampup(epoch) *
mean((sigmoid(-k tanh head) - softmax(logits))^2) over all slices, SGD + poly LR).  Scenarios, seeds and shapes come from
tests/dtc_ref.py, weights from ``oracle.recipe.fill`` over the module's own shape table.  Recorded (arrays and key names only):
  * ``keys`` / ``shapes``: the module's state_dict key list and tensor shapes;
  * ``fwd_tanh`` / ``fwd_logits``: one forward at base width 8 on 2 x 1 x 32 x 32;
  * ``scalars32`` [2, 3] = [seg, l_sdf, l_cons] of two consecutive steps (2 + 2 slices, C = 5, 32 x 32, epoch 20: ramp-up weight
    exp(-1.25) = 0.2865) in fp32, ``post32_*`` = decoder.fc1.0.weight, decoder.fc2.weight, encoder.pre_conv.weight after the second;
    ``scalars64`` / ``post64_*``: the same replay in fp64;
  * ``sdf{i}_labels`` (uint8), ``sdf{i}_d2`` (int32), ``sdf{i}_sdf`` (the scipy fp64 value rounded once to fp32; the 256 x 256 map keeps
    every ``SDF_STRIDE``-th pixel of both axes of d2 and sdf) for the label maps of ``dtc_ref.SDF_FIXTURE``.
The second step passes through sigmoid(-1500 t), whose slope of 375 near t = 0 magnifies rounding differences in t.  The distance
between the fp32 and the fp64 replay of that step, as this generator measured and printed it:
    second-step scalars: max relative distance 1.0e-06   -> bar of the GPU test max(4 x, 2e-2) = 2e-2
    weights after it:    max rel_err           9.5e-05   -> bar of the GPU test max(4 x, 2e-2) = 2e-2
(the GPU test recomputes both from the fixture and prints them).
Those bars are wider than everything two steps at this learning rate change (the update itself is 1.4e-3 / 2.1e-3 / 6.5e-3 of the three
weight tensors), so the GPU test also compares the UPDATE: rel_err(w_after - w_init, post32 - w_init) per tensor for fc1 / fc2 / pre_conv,
bar 0.1.  As this generator measured and printed it (fp32 CPU replays of a wrong trainer against the committed ``post32_*``):
    the fp64 replay (the size of rounding):  1.1e-03 / 3.1e-05 / 1.5e-02   -> passes
    lr = 0 (no backward or no optimizer step): 1.0  / 1.0     / 1.0       -> fails on all three
    beta = 0 (L_sdf dropped from the total):   0.78 / 1.0e-03 / 0.27      -> fails on fc1 and pre_conv
    consistency = 0 (L_cons or its ramp-up dropped): 0.35 / 0.31 / 0.43   -> fails on all three
0.1 is more than six times the fp32 / fp64 distance of the update and less than half the smallest figure a dropped term gives."""
import os
import sys

import numpy as np
import torch
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SMSUT_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from network.dtc import UNet                       # noqa: E402  (reference)
from misc.loss import DiceAndCrossEntropyLoss      # noqa: E402  (reference)

import dtc_ref as R                                # noqa: E402  (ours)
from oracle import recipe                          # noqa: E402  (ours)

torch.set_num_threads(8)
POST = {"fc1": "decoder.fc1.0.weight", "fc2": "decoder.fc2.weight", "pre": "encoder.pre_conv.weight"}


def npy(t):
    return t.detach().cpu().numpy().copy()


def scipy_sdf(labels, n_classes):
    """(d2 int32, sdf fp64) [B, C, H, W] from scipy's transform, with the rules of tests/dtc_ref.py"""
    labels = np.asarray(labels)
    b, h, w = labels.shape
    d2 = np.zeros((b, n_classes, h, w), dtype=np.int32)
    out = np.zeros((b, n_classes, h, w), dtype=np.float64)
    for i in range(b):
        for c in range(n_classes):
            p = labels[i] == c
            if not p.any():
                out[i, c] = 1.0
                continue
            if p.all():
                out[i, c] = -1.0
                continue
            inside, outside = ndimage.distance_transform_edt(p), ndimage.distance_transform_edt(~p)
            d2[i, c] = np.rint(np.where(p, inside, outside) ** 2).astype(np.int32)
            dd = d2[i, c].astype(np.float64)
            v = np.where(p, -np.sqrt(dd) / np.sqrt(dd[p].max()), np.sqrt(dd) / np.sqrt(dd[~p].max()))
            v[p & (d2[i, c] == 1)] = 0.0
            out[i, c] = v
    return d2, out


def fresh(dtype):
    net = UNet(1, R.C, R.WIDTH, "instance", "lrelu")
    sd_ref = net.state_dict()
    shapes = R.shapes()
    assert list(sd_ref.keys()) == list(shapes.keys()), "dtc_ref.shapes() != reference state_dict"
    for k, v in sd_ref.items():
        assert tuple(v.shape) == tuple(shapes[k]), (k, tuple(v.shape), shapes[k])
    net.load_state_dict(recipe.fill(shapes, R.SEED_NET))
    return net.to(dtype).train()


def replay(dtype, lr=R.LR, beta=R.BETA, consistency=R.CONSISTENCY):
    net = fresh(dtype)
    crit = DiceAndCrossEntropyLoss(0.5, 0.5, batch_dice=True)
    opt = torch.optim.SGD(net.parameters(), lr=lr, momentum=R.MOMENTUM, weight_decay=R.WD)
    weight = consistency * R.rampup(R.EPOCH, R.RAMPUP)
    scal = []
    for k, seed in enumerate(R.STEP_SEEDS):
        it = R.IT0 + k
        img, msk = R.step_inputs(seed)
        d2, sdf = scipy_sdf(msk.numpy(), R.C)
        assert np.array_equal(d2, R.edt_sq(msk.numpy(), R.C)) and np.abs(sdf - R.sdf(msk.numpy(), R.C)[1]).max() < 1e-12
        sdf = torch.from_numpy(sdf).to(dtype)
        t, z = net(img.to(dtype))
        seg = crit(z[:R.BS], msk)
        l_sdf = ((t[:R.BS] - sdf) ** 2).mean()
        l_cons = ((torch.sigmoid(-R.K * t) - torch.softmax(z, dim=1)) ** 2).mean()
        total = seg + beta * l_sdf + weight * l_cons
        opt.zero_grad(); total.backward(); opt.step()
        for g in opt.param_groups:
            g["lr"] = lr * (1.0 - it / R.MAX_IT) ** 0.9
        scal.append([seg.item(), l_sdf.item(), l_cons.item()])
    sd = net.state_dict()
    return np.array(scal, dtype=np.float64), {k: npy(sd[v]).astype(np.float64) for k, v in POST.items()}


def main():
    rec = dict(C=R.C, width=R.WIDTH, H=R.SIZE, bs=R.BS, epoch=R.EPOCH, it0=R.IT0)
    net = fresh(torch.float32)
    sd = net.state_dict()
    rec["keys"] = np.array(list(sd.keys()))
    rec["shapes"] = np.array([list(v.shape) + [0] * (4 - v.dim()) for v in sd.values()], dtype=np.int64)
    with torch.no_grad():
        t, z = net(R.fwd_input())
    assert float(t.abs().max()) <= 1.0
    rec["fwd_tanh"], rec["fwd_logits"] = npy(t), npy(z)

    s32, p32 = replay(torch.float32)
    s64, p64 = replay(torch.float64)
    rec["scalars32"], rec["scalars64"] = s32, s64
    for k in POST:
        rec["post32_" + k], rec["post64_" + k] = p32[k].astype(np.float32), p64[k]
    d_scal = float((np.abs(s32[1] - s64[1]) / np.abs(s64[1])).max())
    d_w = max(float(np.abs(p32[k] - p64[k]).max() / np.abs(p64[k]).max()) for k in POST)
    print("fp32 vs fp64 replay: first-step scalars rel %.1e, second-step scalars rel %.1e, weights rel_err %.1e"
          % (float((np.abs(s32[0] - s64[0]) / np.abs(s64[0])).max()), d_scal, d_w))
    print("bars of the GPU test: scalars %.1e, weights %.1e" % (max(4 * d_scal, 2e-2), max(4 * d_w, 2e-2)))

    # what the update assertion of the GPU test sees: rel_err(w_after - w_init, post32 - w_init) of a wrong trainer, per tensor
    init = {k: recipe.fill(R.shapes(), R.SEED_NET)[v].numpy().astype(np.float64) for k, v in POST.items()}
    upd = lambda p: {k: float(np.abs((p[k] - init[k]) - (p32[k] - init[k])).max() / np.abs(p32[k] - init[k]).max()) for k in POST}
    print("update rel_err of the fp64 replay:", upd(p64))
    for name, kw in (("lr = 0", dict(lr=0.0)), ("beta = 0", dict(beta=0.0)), ("consistency = 0", dict(consistency=0.0))):
        print("update rel_err with %s:" % name, upd(replay(torch.float32, **kw)[1]))
    print("size of the update, rel_err(post32, init):", {k: float(np.abs(p32[k] - init[k]).max() / np.abs(init[k]).max()) for k in POST})

    for i, (pat, b, c, h, w) in enumerate(R.SDF_FIXTURE):
        lab = R.label_pattern(pat, b, c, h, w, seed=50 + i)
        d2, sdf = scipy_sdf(lab, c)
        st = R.SDF_STRIDE if h * w > 128 * 128 else 1
        rec[f"sdf{i}_labels"], rec[f"sdf{i}_d2"] = lab.astype(np.uint8), d2[:, :, ::st, ::st]
        rec[f"sdf{i}_sdf"] = sdf[:, :, ::st, ::st].astype(np.float32)

    path = os.path.join(HERE, "dtc.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")
    print("scalars32", s32, "\nscalars64", s64)


if __name__ == "__main__":
    main()
