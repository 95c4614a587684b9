#!/usr/bin/env python3
"""Generator of tests/golden/coranet.npz: the arithmetic of the reference's trainer/coraNetTrainer.py replayed on the CPU with the
REFERENCE's own modules (``network.unet.UNet``, ``misc.loss.SoftDiceLoss``) and torch's ``nn.CrossEntropyLoss(weight=...)``.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_coranet_golden.py

Same method as ``gen_siblings`` of make_golden.py.  The trainer module itself is not imported: it needs medpy and uses ``np.long`` /
``np.float``, which current numpy no longer has.  Scenarios, seeds and shapes come from tests/coranet_ref.py; weights from
oracle/recipe.py.  Recorded (arrays and key names only):
  * ``pre``: one pretrain step at iteration 0 (:435-524); ``t500``: one train step at iteration 500 (semi terms off);
    ``t1200``: two consecutive train steps at iterations 1200, 1201 (:228-424) -- per step the six scalars
    [S, dice+ce, con, rad, certain, uncertain] and the pseudo labels / mask fed in (uint8; from the student at its starting
    weights, :189-208), after the last step ``decoder.fc.weight`` and ``encoder.pre_conv.weight`` of student and teacher;
  * ``pred_*``: pred_unlabel on 4 slices; ``val_loss``: one validation batch (:692-727);
  * ``case_*``: the losses of a small logits-only case (inputs: ``coranet_ref.loss_case``), evaluated by the same modules in fp64.
The mask is fed as fp32 (the reference's ``make_data`` hands it over as fp64, which promotes its masked sums; not reproduced)."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SMSUT_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from network.unet import UNet                      # noqa: E402  (reference)
from misc.loss import SoftDiceLoss                 # noqa: E402  (reference)

import coranet_ref as R                            # noqa: E402  (ours)
from oracle import recipe                          # noqa: E402  (ours)

torch.set_num_threads(8)
L = R.L


def load(module, shapes, seed):
    sd_ref = module.state_dict()
    assert list(sd_ref.keys()) == list(shapes.keys()), "recipe key table != reference state_dict"
    for k, v in sd_ref.items():
        assert tuple(v.shape) == tuple(shapes[k]), (k, tuple(v.shape), shapes[k])
    module.load_state_dict(recipe.fill(shapes, seed))
    return module


def npy(t):
    return t.detach().cpu().numpy().copy()


def split(out):
    """the three heads of a [N, 3L+1, H, W] output: shared background channel + L channels each (:289-295)"""
    back = out[:, 0:1]
    return [torch.cat([back, out[:, 1 + k * L:1 + (k + 1) * L]], dim=1) for k in range(3)]


class Losses:
    def __init__(self, dtype=torch.float32):
        self.dice_b, self.dice_s = SoftDiceLoss(batch_dice=True), SoftDiceLoss(batch_dice=False)
        self.ce = nn.CrossEntropyLoss()
        self.ce_px = nn.CrossEntropyLoss(reduction="none", weight=torch.ones(L + 1, dtype=dtype))
        self.con = nn.CrossEntropyLoss(weight=torch.tensor(R.W_CON, dtype=dtype))
        self.rad = nn.CrossEntropyLoss(weight=torch.tensor(R.W_RAD, dtype=dtype))

    def supervised(self, out, msk):
        o0, o1, o2 = split(out)
        cedc = 0.5 * self.dice_b(o0, msk) + 0.5 * self.ce(o0, msk)
        con, rad = self.con(o1, msk), self.rad(o2, msk)
        return (cedc + con + rad) / 4, cedc, con, rad

    def semi(self, out_p, out_ema, plab, mask, cw):
        p, t = split(out_p), split(out_ema)
        dice = self.dice_s(p[0], plab)
        ce = (self.ce_px(p[0], plab) * mask).sum() / (mask.sum() + 1e-16)
        certain = (ce + dice) / 2
        inv = (1 - mask).unsqueeze(1)
        terms = [cw * ((((torch.softmax(a, dim=1) - torch.softmax(b, dim=1)) ** 2) * inv).sum() / (inv.sum() + 1e-16))
                 for a, b in zip(p, t)]
        return certain, (terms[0] + terms[1] + terms[2]) / 3


def pseudo_of(net, img):
    with torch.no_grad():
        o0, o1, o2 = split(net(img))
    plab = torch.argmax(o0, dim=1)
    mask = (torch.argmax(o1, dim=1) == torch.argmax(o2, dim=1))
    return plab, mask.float()


def fresh():
    stu = load(UNet(1, 3 * L + 1, R.WIDTH, "instance", "lrelu"), R.shapes(), R.SEED_STUDENT)
    ema = load(UNet(1, 3 * L + 1, R.WIDTH, "instance", "lrelu"), R.shapes(), R.SEED_TEACHER)
    for p in ema.parameters():
        p.detach_()
    stu.train(); ema.train()
    opt = torch.optim.SGD(stu.parameters(), lr=R.LR, momentum=R.MOMENTUM, weight_decay=R.WD)
    return stu, ema, opt


def ema_step(stu, ema, it):
    alpha = R.ema_alpha(it)
    for ep, p in zip(ema.parameters(), stu.parameters()):
        ep.data.mul_(alpha).add_(p.data, alpha=1 - alpha)


def main():
    crit = Losses()
    rec = dict(L=L, width=R.WIDTH, H=R.SIZE, bs=R.BS, epoch=R.EPOCH)
    cw = 1 * R.rampup(R.EPOCH, 30)

    # ---- pretrain step (iteration 0): supervised loss, SGD, EMA (alpha = 0), no LR change
    it0, seeds = R.SCENARIOS["pre"]
    stu, ema, opt = fresh()
    img1, msk, img2 = R.step_inputs(seeds[0])
    out = stu(torch.cat([img1, img2], 0))                 # the reference forwards both halves and uses the first
    s = crit.supervised(out[:R.BS], msk)
    opt.zero_grad(); s[0].backward(); opt.step()
    ema_step(stu, ema, it0)
    rec["pre_scalars"] = np.array([[v.item() for v in s] + [0.0, 0.0]], dtype=np.float64)
    rec["pre_post_fc"] = npy(stu.state_dict()["decoder.fc.weight"])
    rec["pre_post_ema_fc"] = npy(ema.state_dict()["decoder.fc.weight"])

    # ---- train steps
    for name in ("t500", "t1200"):
        it0, seeds = R.SCENARIOS[name]
        stu, ema, opt = fresh()
        start = load(UNet(1, 3 * L + 1, R.WIDTH, "instance", "lrelu"), R.shapes(), R.SEED_STUDENT).train()
        scal, plabs, masks = [], [], []
        for k, seed in enumerate(seeds):
            it = it0 + k
            img1, msk, img2 = R.step_inputs(seed)
            plab, mask = pseudo_of(start, img2)           # pseudo labels of the student at its starting weights: inputs of the step
            s = crit.supervised(stu(img1), msk)
            out_p = stu(img2)
            with torch.no_grad():
                out_ema = ema(img2)
            certain, uncertain = crit.semi(out_p, out_ema, plab, mask, cw)
            if it < 1000:
                certain, uncertain = torch.tensor(0.0), torch.tensor(0.0)
            loss = s[0] + certain + uncertain * 0.1
            opt.zero_grad(); loss.backward(); opt.step()
            ema_step(stu, ema, it)
            for g in opt.param_groups:
                g["lr"] = R.LR * (1.0 - it / R.MAX_IT) ** 0.9
            scal.append([v.item() for v in s] + [certain.item(), uncertain.item()])
            plabs.append(npy(plab).astype(np.uint8)); masks.append(npy(mask).astype(np.uint8))
        rec[name + "_scalars"] = np.array(scal, dtype=np.float64)
        rec[name + "_plab"], rec[name + "_mask"] = np.stack(plabs), np.stack(masks)
    for tag, net in (("", stu), ("ema_", ema)):
        rec[f"post_{tag}fc"] = npy(net.state_dict()["decoder.fc.weight"])
        rec[f"post_{tag}pre"] = npy(net.state_dict()["encoder.pre_conv.weight"])

    # ---- pred_unlabel on 4 slices (batch of one, :182-217) and the flip rate under the project's parity bar
    stu, _, _ = fresh()
    img, lab = R.pred_inputs()
    plab = torch.cat([pseudo_of(stu, img[i:i + 1])[0] for i in range(img.size(0))])
    mask = torch.cat([pseudo_of(stu, img[i:i + 1])[1] for i in range(img.size(0))])
    rec["pred_plab"], rec["pred_mask"] = npy(plab).astype(np.uint8), npy(mask).astype(np.uint8)
    rec["pred_dice"] = float(np.mean([R.binary_dc(npy(plab[i]), npy(lab[i])) for i in range(img.size(0))]))
    with torch.no_grad():
        z = stu(img)
    noise = torch.from_numpy(np.random.RandomState(7).uniform(-1, 1, tuple(z.shape))).float() * 1e-3 * z.abs().max()
    q2, m2 = R.pseudo(z + noise)
    flips = (float((q2 != plab).float().mean()), float((m2 != mask).float().mean()))
    print("pred_unlabel flips under 1e-3 * max|z| noise: labels %.3f %%, mask %.3f %%" % (100 * flips[0], 100 * flips[1]))
    assert max(flips) <= 0.009, "pick other seeds (the 1 % cap of the GPU test needs head-room)"

    # ---- one validation batch (eval mode)
    stu.eval()
    img, msk = R.val_inputs()
    with torch.no_grad():
        rec["val_loss"] = np.array([v.item() for v in crit.supervised(stu(img), msk)], dtype=np.float64)

    # ---- logits-only case in fp64: what tests/coranet_ref.py must reproduce to 1e-6
    c64 = Losses(torch.float64)
    z, e, y, q, m = R.loss_case()
    rec["case_cw"] = 0.7
    rec["case_sup"] = np.array([v.item() for v in c64.supervised(z.double(), y)], dtype=np.float64)
    for tag, mm in (("", m), ("_m1", torch.ones_like(m)), ("_m0", torch.zeros_like(m))):
        rec["case_semi" + tag] = np.array([v.item() for v in c64.semi(z.double(), e.double(), q, mm.double(), 0.7)], dtype=np.float64)
    qp, mp = pseudo_of(lambda x: x, z)
    rec["case_plab"], rec["case_mask"] = npy(qp).astype(np.uint8), npy(mp).astype(np.uint8)

    path = os.path.join(HERE, "coranet.npz")
    np.savez_compressed(path, **rec)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.1f} KiB")
    for k in ("pre_scalars", "t500_scalars", "t1200_scalars", "val_loss", "case_sup", "case_semi", "pred_dice"):
        print(k, rec[k])


if __name__ == "__main__":
    main()
