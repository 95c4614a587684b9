"""``meanTeacherTrainer`` (reference trainer/meanTeacherTrainer.py:37-151): student U-Net + EMA teacher, DiceCE on
the labeled half, softmax-MSE consistency between the student on the unlabeled half and the teacher on a noised
copy (from iteration 100 on), SGD + poly LR, EMA update after every step.  Same kernels as the U-Net path plus
``ops.softmax_mse``."""
import torch

from .. import config as cfg
from .. import ops, parallel
from ..network.unet import UNet
from .baseTrainer import BaseTrainer, make_parser, make_sgd, run_main


class meanTeacherTrainer(BaseTrainer):
    def __init__(self, phase, args=None):
        super().__init__(phase, args)
        self.lambda_semi = 1          # :41
        self.ema_decay = 0.99
        self.epoch_rampup = 30
        self.alpha = 0
        self.semi_start_iter = 100    # :123
        self.log_step = 50

    def build_network(self):
        mk = lambda: UNet(cfg.img_channels, cfg.n_label + 1, cfg.base_width, norm_type="instance", act_type="lrelu").to(self.device)
        self.net = mk()
        parallel.broadcast_parameters(self.net, self.group)
        if self.phase == "train":
            self.ema = self.build_teacher(mk)
            self.optimizer = make_sgd(self.net.parameters(), cfg.lr, 0.9, cfg.weight_decay)
            self.reducer = parallel.GradAllReducer(self.net.parameters(), self.group)

    def update_ema_variable(self):
        """:63-69 -- ema = alpha * ema + (1 - alpha) * student, alpha = 0 for the first 100 iterations."""
        self.alpha = self.ema_alpha()
        ema, cur = list(self.ema.parameters()), [p.detach() for p in self.net.parameters()]
        torch._foreach_mul_(ema, self.alpha)
        torch._foreach_add_(ema, cur, alpha=1 - self.alpha)

    def train_iteration(self, img, msk, noise=None):
        """One iteration of :86-149 on ``img`` = [labeled | unlabeled] (bs + bs slices).  Returns the device tensor
        [seg_loss, semi_loss]."""
        bs = msk.size(0)
        ul_img = img[bs:]
        if noise is None:
            noise = torch.clamp(torch.randn_like(ul_img) * 0.01, -0.02, 0.02)                  # :104
        lambda_semi = self.lambda_semi * self.sigmoid_rampup(self.epoch, self.epoch_rampup)
        with ops.wino_prepared(self.net, self.ema):         # (student: optimizer step; teacher: EMA update -- both after)
            out = self.net(img)
            with torch.no_grad():
                ema_out = self.ema(ul_img + noise)
            seg = self.loss(out[:bs], msk)
            if self.iter < self.semi_start_iter:
                semi = torch.zeros((), device=self.device)
            else:
                semi = ops.softmax_mse(out[bs:], ema_out)                                         # :129-131
            total = seg + lambda_semi * semi
            self.optimizer.zero_grad(set_to_none=True)
            total.backward()
        self.reducer.reduce()
        self.optimizer.step()
        self.update_ema_variable()
        self.set_poly_lr(self.optimizer)
        self.iter += 1
        return torch.stack([seg.detach(), semi.detach()])

    train_epoch = BaseTrainer.lb_ul_epoch

    def _log_step(self, i, scal):
        self.info("Iter %d, global_iter: %d, semi_loss: %.4f, seg_loss: %.4f, alpha: %f"
                  % (i, self.iter, scal[1].item(), scal[0].item(), self.alpha))


def main(argv=None):
    run_main(meanTeacherTrainer, make_parser(("train", "test")), argv)


if __name__ == "__main__":
    main()
