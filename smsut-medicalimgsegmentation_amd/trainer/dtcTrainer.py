"""``dtcTrainer``: dual-task consistency (DTC, Luo et al. 2021) on the reference's ``network/dtc.py`` U-Net -- the one network module of
the reference that ships without a trainer.  Modelled on ``meanTeacherTrainer`` without the teacher: DiceCE on the labelled half's
logits, an MSE between the tanh head and the normalised signed distance map of every class of every labelled slice, and on all slices
the consistency ``mean((sigmoid(-k * tanh_out) - softmax(logits)) ** 2)`` between the two tasks, ramped up over ``epoch_rampup`` epochs.
The signed distance maps are recomputed every iteration from the (augmented) labels ON THE DEVICE (``ops.signed_distance_map``,
csrc/dtc.hip) -- the published code does that with scipy on the host -- and both DTC terms with their gradients come from the fused
``ops.dtc_loss``.  SGD + poly LR as the sibling baselines."""
import torch

from .. import config as cfg
from .. import ops, parallel
from ..network.dtc import UNet
from .baseTrainer import BaseTrainer, make_parser, make_sgd, run_main, sgd_step


class dtcTrainer(BaseTrainer):
    def __init__(self, phase, args=None):
        super().__init__(phase, args)
        self.beta = 0.3               # weight of the level-set regression (published DTC value)
        self.k = 1500                 # steepness of the level-set -> probability transform sigmoid(-k t)
        self.consistency = 1.0
        self.epoch_rampup = 40        # consistency_rampup
        self.log_step = 50

    def build_network(self):
        self.net = UNet(cfg.img_channels, cfg.n_label + 1, cfg.base_width, norm_type="instance", act_type="lrelu").to(self.device)
        parallel.broadcast_parameters(self.net, self.group)
        if self.phase == "train":
            self.optimizer = make_sgd(self.net.parameters(), cfg.lr, 0.9, cfg.weight_decay)
            self.reducer = parallel.GradAllReducer(self.net.parameters(), self.group)

    def _forward_eval(self, img):
        """Validation and ``-p test`` score the segmentation head."""
        return self.net(img)[1]

    def train_iteration(self, img, msk):
        """One iteration on ``img`` = [labelled | unlabelled] (bs + bs slices), ``msk`` int64 [bs, H, W]:
        total = DiceCE(z[:bs], msk) + beta * L_sdf + consistency * rampup(epoch) * L_cons.  Every term is a local mean, so under data
        parallelism the averaging gradient all-reduce is all it needs.  Returns the device tensor [seg, l_sdf, l_cons]."""
        bs = msk.size(0)
        weight = self.consistency * self.sigmoid_rampup(self.epoch, self.epoch_rampup)
        with ops.wino_prepared(self.net):
            t, z = self.net(img)
            sdf = ops.signed_distance_map(msk, z.size(1))
            seg = self.loss(z[:bs], msk)
            dtc = ops.dtc_loss(t, z, sdf, self.k)
            total = seg + self.beta * dtc[0] + weight * dtc[1]
            self.optimizer.zero_grad(set_to_none=True)
            total.backward()
        self.reducer.reduce()
        sgd_step(self.optimizer)
        self.set_poly_lr(self.optimizer)
        self.iter += 1
        return torch.cat([seg.detach().reshape(1), dtc.detach()])

    train_epoch = BaseTrainer.lb_ul_epoch

    def _meter_step(self, meter, scal, modal, n):
        super()._meter_step(meter, scal, modal, n)
        # the host has just waited for the scalars, so reading the bad-label word costs no extra wait: a label outside
        # [0, C) raises here.  A caller that passes no meter never waits for the device in this loop and is NOT checked
        # (such a pixel then simply belongs to no class); it can call ops.sdf_check() itself wherever it synchronises.
        ops.sdf_check(self.device)

    def _log_step(self, i, scal):
        s = scal.tolist()
        self.info("Iter %d, global_iter: %d, seg_loss: %.4f, sdf_loss: %.4f, consistency_loss: %.4f"
                  % (i, self.iter, s[0], s[1], s[2]))


def main(argv=None):
    run_main(dtcTrainer, make_parser(("train", "test")), argv)


if __name__ == "__main__":
    main()
