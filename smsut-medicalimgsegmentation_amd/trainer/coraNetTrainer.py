"""``coraNetTrainer`` (reference trainer/coraNetTrainer.py:100-744): the stock U-Net with 3 * n_label + 1 output channels -- three
(n_label + 1)-class heads that share the background logit -- as student and EMA teacher.  Pretraining fits the supervised three-head
loss; training adds, on slices pseudo-labelled by the student itself, a Dice + masked CE term where the two auxiliary heads agree
("certain") and a softmax-MSE consistency with the teacher where they do not ("uncertain").  The convolutional path is the U-Net's;
everything after the logits runs in the fused head kernels of csrc/coranet.hip (``ops.cora_sup_loss``, ``ops.cora_semi_loss``,
``ops.cora_pseudo``, ``ops.ema_update``): no head is ever concatenated out of the logits."""
import time
from os.path import join as pjoin

import numpy as np
import torch

from .. import config as cfg
from .. import ops, parallel
from ..network.unet import UNet
from . import baseTrainer
from .baseTrainer import BaseTrainer, LoaderCycle, make_sgd, run_main, sgd_step

SCALARS = ("supervised", "dice_ce", "con", "rad", "certain", "uncertain")


class PseudoBatches:
    """The reference's ``DataLoader(make_data(...), batch_size, shuffle=True, drop_last=True)`` (:224-225) over tensors that stay on
    the device: every ``iter()`` draws a new order and yields ``(img [bs,1,H,W], plab int64 [bs,H,W], mask fp32 [bs,H,W], lab, mdl)``."""

    def __init__(self, img, plab, mask, lab, mdl, batch_size):
        self.img, self.plab, self.mask, self.lab, self.mdl, self.bs = img, plab, mask, lab, mdl, batch_size

    def __len__(self):
        return self.img.size(0) // self.bs

    def __iter__(self):
        order = torch.randperm(self.img.size(0))
        for b in range(len(self)):
            idx = order[b * self.bs:(b + 1) * self.bs]
            di = idx.to(self.img.device)
            yield self.img[di], self.plab[di], self.mask[di], self.lab[di], self.mdl[idx]


class coraNetTrainer(BaseTrainer):
    def __init__(self, phase, args=None):
        super().__init__(phase, args)
        self.lambda_semi = 1          # :104
        self.ema_decay = 0.99
        self.epoch_rampup = 30
        self.alpha = 0
        self.semi_start_iter = 1000   # :344
        self.model_id = getattr(args, "model_id", None)
        self.log_step = 50
        self._pseudo = None

    def build_network(self):
        mk = lambda: UNet(cfg.img_channels, 3 * cfg.n_label + 1, cfg.base_width, norm_type="instance", act_type="lrelu").to(self.device)
        self.net = mk()
        parallel.broadcast_parameters(self.net, self.group)
        vec = lambda pair: torch.tensor(cfg.class_weights(pair), dtype=torch.float32, device=self.device)
        self.w_con, self.w_rad = vec(cfg.w_con), vec(cfg.w_rad)
        if self.phase == "train":
            self.ema = self.build_teacher(mk)
            self.optimizer = make_sgd(self.net.parameters(), cfg.lr, 0.9, cfg.weight_decay)
            self.reducer = parallel.GradAllReducer(self.net.parameters(), self.group)

    # ------------------------------------------------------------------ teacher
    def update_ema_variable(self):
        """:168-174 -- ema = alpha * ema + (1 - alpha) * student in one launch; alpha = 0 for the first 100 iterations."""
        self.alpha = self.ema_alpha()
        ops.ema_update(self.ema.parameters(), self.net.parameters(), self.alpha)

    def save_ema_model(self, prefix):
        if self.rank == 0:
            path = pjoin(self.expr_root, self.model_idx, "ckpt", f"{prefix}.ckpt")
            torch.save({k: v.contiguous() for k, v in self.ema.state_dict().items()}, path)
            self.info(f"Save model to {path}.")

    def load_ema_model(self, model_idx=None, which_ckpt="last"):
        path = pjoin(self.expr_root, model_idx or self.model_idx, "ckpt", f"{which_ckpt}.ckpt")
        self.ema.load_state_dict(torch.load(path, map_location="cpu"))
        self.info(f"Load model from {path}.")

    # ------------------------------------------------------------------ steps
    def poly_lr(self):
        """:420 -- the training phase decays over ``cora_epoch`` epochs, not ``max_epoch``."""
        return cfg.lr * (1.0 - self.iter / (cfg.cora_epoch * cfg.num_iter_per_epoch)) ** 0.9

    def sup_loss(self, out, msk):
        """[S, dice+ce of head 0, con, rad] (:288-301); batch statistics go through the one-all-reduce route under data parallelism."""
        return ops.cora_sup_loss(out, msk, self.w_con, self.w_rad, cfg.weight_ce, cfg.weight_dc, self.group)

    def _step(self, total):
        self.optimizer.zero_grad(set_to_none=True)
        total.backward()

    def pretrain_iteration(self, img, msk):
        """One iteration of ``pre_epoch`` (:435-524): supervised loss, SGD step, EMA update, NO learning-rate change.  The reference
        forwards the unlabelled half too and ignores its output; with InstanceNorm (per-sample statistics) that half cannot influence
        the labelled half, so only the labelled half is forwarded here.  Returns the device tensor [S, dice+ce, con, rad]."""
        with ops.wino_prepared(self.net):
            sup = self.sup_loss(self.net(img), msk)
            self._step(sup[0])
        self.reducer.reduce()
        sgd_step(self.optimizer)
        self.update_ema_variable()
        self.iter += 1
        return sup.detach()

    def train_iteration(self, img1, msk, img2, plab, mask):
        """One iteration of ``train_epoch`` (:228-424): labelled ``img1`` / ``msk``; ``img2`` with its pseudo labels ``plab`` (int64) and
        certainty mask ``mask`` (fp32 0/1) from ``pred_unlabel``.  total = S + certain + 0.1 * uncertain, the last two exactly 0 and
        without gradient while ``iter < 1000`` (the student then skips ``img2``: its output would not reach the loss).  The two
        student passes run as one 2*bs pass (InstanceNorm: the halves cannot see each other); the teacher sees ``img2`` itself (the
        reference draws a noise tensor at :284 and never uses it).  Returns the device tensor
        [S, dice+ce, con, rad, certain, uncertain]."""
        bs = img1.size(0)
        semi_on = self.iter >= self.semi_start_iter
        cw = self.lambda_semi * self.sigmoid_rampup(self.epoch, self.epoch_rampup)
        with ops.wino_prepared(self.net, self.ema):          # (student: optimizer step; teacher: EMA update -- both after)
            if semi_on:
                out = self.net(torch.cat([img1, img2], 0))
                with torch.no_grad():
                    ema_out = self.ema(img2)
                sup = self.sup_loss(out[:bs], msk)
                semi = ops.cora_semi_loss(out[bs:], ema_out, plab, mask, cw)          # [certain, uncertain]
                total = sup[0] + semi[0] + 0.1 * semi[1]
            else:
                sup = self.sup_loss(self.net(img1), msk)
                semi = torch.zeros(2, device=self.device)
                total = sup[0]
            self._step(total)
        self.reducer.reduce()
        sgd_step(self.optimizer)
        self.update_ema_variable()
        self.set_poly_lr(self.optimizer)
        self.iter += 1
        return torch.cat([sup.detach(), semi.detach()])

    # ------------------------------------------------------------------ pseudo labels
    @torch.no_grad()
    def pred_unlabel(self, ul_loader):
        """:176-226 -- pseudo labels = argmax of head 0, certainty mask = (argmax of head 1 == argmax of head 2), for every slice of
        ``ul_loader``, in batches of ``cfg.batch_size`` on the device (per-sample normalisation makes this equal to the reference's
        batch of one).  Images, pseudo labels and masks stay on the device.  Returns (a shuffled, drop-last batch source over them,
        the mean over slices of the pseudo labels' binary Dice against the loader's labels -- ``misc.utils.binary_dc`` per slice)."""
        imgs, plabs, masks, labs, mdls = [], [], [], [], []
        for img, lab, mdl, _ in ul_loader:
            imgs.append(img.to(self.device)); labs.append(lab.to(self.device)); mdls.append(torch.as_tensor(mdl).reshape(-1).cpu())
        img, lab, mdl = torch.cat(imgs), torch.cat(labs), torch.cat(mdls)
        bs = cfg.batch_size
        with ops.wino_prepared(self.net, forms="f"):
            for i in range(0, img.size(0), bs):
                q, m = ops.cora_pseudo(self.net(img[i:i + bs]))
                plabs.append(q); masks.append(m)
        plab, mask = torch.cat(plabs), torch.cat(masks)
        a, b = plab > 0, lab > 0
        den = (a.sum((1, 2)) + b.sum((1, 2))).double()
        dice = torch.where(den > 0, 2.0 * (a & b).sum((1, 2)).double() / den.clamp(min=1), torch.zeros_like(den)).mean().item()
        self.info("Pseudo label dice : {}".format(dice))
        return PseudoBatches(img, plab, mask, lab, mdl, bs), dice

    # ------------------------------------------------------------------ epochs
    def pre_epoch(self, lb_loader, ul_loader, meter):
        self.net.train()
        lb = LoaderCycle(lb_loader)
        for i in range(cfg.num_iter_per_epoch):
            img1, msk, mdl1, _ = next(lb)
            scal = self.pretrain_iteration(img1.to(self.device, non_blocking=True), msk.to(self.device, non_blocking=True))
            if meter is not None:
                v, n = meter.collect_loss_by(scal[0].item(), mdl1[0].item(), 2 * img1.size(0))
                meter.accumulate(v, n)
            if (i + 1) % self.log_step == 0:
                s = scal.tolist()
                self.info("Iter %d, global_iter: %d, train_loss: %.4f cedc_loss: %.4f, loss_con: %.4f, loss_rad: %.4f"
                          % (i, self.iter, s[0], s[1], s[2], s[3]))

    def train_epoch(self, lb_loader, ul_loader, meter, new_loader=None):
        new_loader = new_loader if new_loader is not None else self._pseudo
        if new_loader is None:
            raise RuntimeError("coraNetTrainer.train_epoch needs the pseudo-labelled batches of pred_unlabel()")
        self.net.train(); self.ema.train()
        lb, pse = LoaderCycle(lb_loader), LoaderCycle(new_loader)
        for i in range(cfg.num_iter_per_epoch):
            img1, msk, mdl1, _ = next(lb)
            img2, plab, mask, _, _ = next(pse)
            scal = self.train_iteration(img1.to(self.device, non_blocking=True), msk.to(self.device, non_blocking=True), img2, plab, mask)
            if meter is not None:
                s = scal.tolist()
                v, n = meter.collect_loss_by(s[0] + s[4] + 0.1 * s[5], mdl1[0].item(), 2 * img1.size(0))
                meter.accumulate(v, n)
            if (i + 1) % self.log_step == 0:
                s = scal.tolist()
                self.info("Iter %d, global_iter: %d, supervised_loss: %.4f, certain_loss: %.4f, uncertain_loss: %f"
                          % (i, self.iter, s[0], s[4], s[5]))

    def prefit(self, loader_type="synthetic", max_epoch=None):
        """:526-602 -- ``cfg.pre_epoch`` epochs of the supervised three-head loss; the best validation Dice writes ``pre_best`` /
        ``pre_ema_best``, the end ``pre_last`` / ``pre_ema_last``."""
        lb, ul, test = self.get_loaders(loader_type)
        self.adopt_train_loaders(lb, ul)
        train_meter, test_meter = self._meters()
        n_epochs = max_epoch or cfg.pre_epoch
        tic = time.time()
        for epoch in range(n_epochs):
            train_meter.reset_cur()
            self.pre_epoch(lb, ul, train_meter)
            self.epoch += 1
            train_meter.update_cur()
            self.info("[TRN] pre Epoch: %d/%d, elapsed: %.2fs,%s" % (epoch, n_epochs, time.time() - tic, train_meter))
            tic = time.time()
            if self._validate(test, test_meter, "pre ", epoch, n_epochs, tic):
                self.save_model(prefix="pre_best")
                self.save_ema_model(prefix="pre_ema_best")
        if self._agree(self.model_idx is not None):
            self.save_model(prefix="pre_last")
            self.save_ema_model(prefix="pre_ema_last")

    def fit(self, loader_type="synthetic", max_epoch=None):
        """:604-690 -- load ``pre_best`` / ``pre_ema_best`` of run ``--model_id`` (this trainer's own run directory when none is
        given), pseudo-label the unlabelled slices, then ``cfg.cora_epoch`` epochs that re-predict every ``cfg.pred_step``."""
        lb, ul, test = self.get_loaders(loader_type)
        self.adopt_train_loaders(lb, ul)
        train_meter, test_meter = self._meters()
        src = self.model_id or self.model_idx
        self.load_model(src, "pre_best")
        self.load_ema_model(src, "pre_ema_best")
        self.net.to(self.device); self.ema.to(self.device)
        n_epochs = max_epoch or cfg.cora_epoch
        tic = time.time()
        for epoch in range(n_epochs):
            if epoch % cfg.pred_step == 0:
                self._pseudo, _ = self.pred_unlabel(ul)
            train_meter.reset_cur()
            self.train_epoch(lb, ul, train_meter, self._pseudo)
            self.epoch += 1
            train_meter.update_cur()
            self.info("lr: %g." % self.optimizer.param_groups[0]["lr"])
            self.info("[TRN] Epoch: %d/%d, elapsed: %.2fs,%s" % (epoch, n_epochs, time.time() - tic, train_meter))
            tic = time.time()
            if self._validate(test, test_meter, "", epoch, n_epochs, tic):
                self.save_model(prefix="best")
        if self._agree(self.model_idx is not None):
            self.save_model(prefix="last")

    # ------------------------------------------------------------------ evaluation: the three-head loss, head 0 predicts (:692-744)
    def _eval_loss(self, out, msk):
        return self.sup_loss(out, msk)[0]

    def _eval_classes(self, out):
        """Head 0 is channels 0 .. L of the 3L+1."""
        return (out.shape[1] - 1) // 3 + 1

    def _eval_pred(self, out):
        return ops.cora_pseudo(out)[0]

    def save_pseudo(self, loader_type, expr_root):
        """``-p pseudo``: pseudo labels and certainty masks of the unlabelled slices as ``pseudo/{plab,mask}.npy`` (uint8)."""
        from ..misc.utils import maybe_mkdir
        _, ul, _ = self.get_loaders(loader_type)
        src, dice = self.pred_unlabel(ul)
        root = pjoin(expr_root, "pseudo")
        maybe_mkdir(root)
        np.save(pjoin(root, "plab.npy"), src.plab.to(torch.uint8).cpu().numpy())
        np.save(pjoin(root, "mask.npy"), src.mask.to(torch.uint8).cpu().numpy())
        return dice


def make_parser():
    return baseTrainer.make_parser(("pretrain", "train", "test", "pseudo"),
                                   model_id_help="run to load: pre_best / pre_ema_best for train, --which_ckpt for test / pseudo")


def main(argv=None):
    # the reference's main has its prefit() call commented out (:764): the phase name `pretrain` is ours; it builds the same trainer
    run_main(coraNetTrainer, make_parser(), argv, extra={"pretrain": "prefit", "pseudo": "save_pseudo"}, build_as={"pretrain": "train"})


if __name__ == "__main__":
    main()
