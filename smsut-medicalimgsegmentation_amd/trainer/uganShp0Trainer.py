"""``UGANShp0Trainer`` pieces inherited by the consistency trainer (reference trainer/uganShp0Trainer.py:36-287):
``build_network`` (UGANnce + Discriminator + PatchNCE, SGD / Adam), ``load_model`` / ``save_model`` with the
``{prefix}_G.ckpt`` / ``{prefix}_D.ckpt`` names, ``label2onehot``, ``create_vectors``, ``denorm``,
``gradient_penalty`` and the ``val_phase`` validation forward."""
from os.path import join as pjoin

import numpy as np
import torch

from .. import config as cfg
from .. import ops, parallel
from ..network.patchnce import PatchNCELoss
from ..network.ugan import Discriminator, UGANnce
from .baseTrainer import BaseTrainer, make_adam, make_sgd


class UGANShp0Trainer(BaseTrainer):
    def __init__(self, phase, args=None):
        self.lambda_cls, self.lambda_rec, self.lambda_gp, self.lambda_seg = 1, 10, 10, 10     # :39-42
        self.log_step, self.n_critic = 50, 1
        self.beta1, self.beta2 = 0.9, 0.999
        super().__init__(phase, args)

    def build_network(self):
        self.net = UGANnce(cfg.img_channels, cfg.n_label + 1, cfg.n_modal, cfg.base_width).to(self.device)
        self.criterionNCE = [PatchNCELoss(cfg.batch_size) for _ in cfg.nce_layers]                 # :57-59
        self.D = Discriminator(cfg.input_size, cfg.n_modal, cfg.base_width,
                               max_width=256 if cfg.base_width == 16 else 512).to(self.device)     # :61-63
        parallel.broadcast_parameters(self.net, self.group)
        parallel.broadcast_parameters(self.D, self.group)
        if self.phase == "train":
            self.optimizer = make_sgd(self.net.parameters(), cfg.lr, 0.9, cfg.weight_decay)
            self.d_optimizer = make_adam(self.D.parameters(), cfg.lr, [self.beta1, self.beta2], cfg.weight_decay)
            self.g_reducer = parallel.GradAllReducer(self.net.parameters(), self.group)
            self.d_reducer = parallel.GradAllReducer(self.D.parameters(), self.group)

    def load_model(self, model_idx, which_ckpt):
        root = pjoin(self.expr_root, model_idx, "ckpt")
        self.net.load_state_dict(torch.load(pjoin(root, f"{which_ckpt}_G.ckpt"), map_location="cpu"))
        self.D.load_state_dict(torch.load(pjoin(root, f"{which_ckpt}_D.ckpt"), map_location="cpu"))
        self.net.to(self.device); self.D.to(self.device)
        self.info(f"[*] Load G and D from {root}.")

    def save_model(self, prefix):
        if self.rank == 0:
            root = pjoin(self.expr_root, self.model_idx, "ckpt")
            # .contiguous(): checkpoints hold plain OIHW tensors, loadable by the reference's nn.Modules
            torch.save({k: v.contiguous() for k, v in self.net.state_dict().items()}, pjoin(root, f"{prefix}_G.ckpt"))
            torch.save({k: v.contiguous() for k, v in self.D.state_dict().items()}, pjoin(root, f"{prefix}_D.ckpt"))
            self.info(f"[*] Save G and D to {root}.")
        self.save_train_state(prefix)                       # collective under DP: every rank's RNG / loader state

    def label2onehot(self, modals, dim=cfg.n_modal):
        out = torch.zeros(modals.size(0), dim)
        out[np.arange(modals.size(0)), modals.long().cpu()] = 1
        return out

    def create_vectors(self, vec_org, dim):
        return [self.label2onehot(torch.ones(vec_org.size(0)) * i, dim).to(self.device) for i in range(dim)]

    @staticmethod
    def denorm(x):
        return ((x + 1.0) / 2.0).clamp_(0, 1)

    def gradient_penalty(self, y, x):
        """:127-134 -- ``create_graph=True`` so ``d_loss.backward()`` differentiates D's backward again.  The
        ``input_grads_only`` scope tells the HIP backward ops that only d/dx is wanted here."""
        weight = torch.ones(y.size(), device=self.device)
        with ops.input_grads_only():
            dydx = torch.autograd.grad(outputs=y, inputs=x, grad_outputs=weight, retain_graph=True, create_graph=True,
                                       only_inputs=True)[0]
        return ops.grad_penalty(dydx)

    def _forward_eval(self, img):
        seg, _ = self.net(img, val_phase=True)            # :267
        return seg

    # ------------------------------------------------------------------ translation metrics of the test phase (cfg.test_translation)
    def test(self, loader_type, expr_root):
        """The base ``test``; with ``cfg.test_translation`` also ``translation_report`` over a fresh test loader."""
        mo = super().test(loader_type, expr_root)
        if cfg.test_translation:
            _, _, loader = self.get_loaders(loader_type)
            self.translation_report(loader, expr_root)
        return mo

    @staticmethod
    def translation_partners():
        """{modality id: the ids it is paired with} from ``cfg.test_translation_pairs``, both directions; a pair that names a
        modality ``cfg.Modality`` does not have is skipped."""
        names_of = cfg.Modality.__members__
        partner = {}
        for pa, pb in cfg.test_translation_pairs:
            if pa in names_of and pb in names_of:
                ia, ib = names_of[pa].value, names_of[pb].value
                partner.setdefault(ia, []).append(ib)
                partner.setdefault(ib, []).append(ia)
        return partner

    def translation_report(self, loader, expr_root):
        """SSIM / PSNR / MAE of the unified translator over ``loader`` (batches ``(img, msk, modality ids, names 'm_pid_z')``), in
        ``net.eval()`` under ``no_grad`` through the ``val_phase`` forward (netF is not involved); images are compared after
        ``denorm`` (range [0, 1], data_range 1).  Two sets of [n_modal, n_modal] tables, row = source modality i, column = j:
          cycle   denorm(x) against denorm(G(G(x, e_j - e_i), e_i - e_j)), the diagonal (zero vector both times) included;
          paired  for each pair (a, b) of ``cfg.test_translation_pairs``, in both directions, denorm(G(x_a, e_b - e_a)) against
                  denorm(x_b) for every slice 'a_pid_z' whose partner 'b_pid_z' is in the loader too (the real slices and the
                  translations of the paired modalities are kept on the device, keyed by name); cells without data are NaN, a
                  pair naming an unknown modality is skipped.
        Writes ``{modality}_translation_matrix.csv`` -- cycle SSIM, PSNR, MAE, then paired SSIM, PSNR, MAE, '%.4f' rows separated
        by ',' with an empty line between blocks -- logs it, and returns ``{table: (ssim, psnr, mae)}``.  Every comparison is one
        ``ops.image_similarity`` launch whose rows stay on the device (``TranslationMeter``): nothing is read back before the
        loader is exhausted, then one stacked copy."""
        from ..misc.utils import TranslationMeter, maybe_mkdir, translation_text
        self.net.eval()
        meter = TranslationMeter(data_range=1.0)
        partner = self.translation_partners()
        real, translated = {}, []                          # name -> denorm(x) slice | (source name, target name, i, j, denorm(G(x)) slice)
        with torch.no_grad():
            for img, _, mdl, inm in loader:
                x = img.to(self.device)
                ids = [int(v) for v in mdl.tolist()]
                inm = list(inm)[:len(ids)]
                vec_org = self.label2onehot(mdl, cfg.n_modal).to(self.device)
                x01 = self.denorm(x)
                groups = {}                                # the batch's slices by source modality (one group with the in-turn loaders)
                for k, i in enumerate(ids):
                    groups.setdefault(i, []).append(k)
                for k, i in enumerate(ids):
                    if i in partner:
                        real[inm[k]] = x01[k]
                for j, vec in enumerate(self.create_vectors(vec_org, cfg.n_modal)):
                    _, fwd = self.net(x, vec - vec_org, val_phase=True)
                    _, back = self.net(fwd, vec_org - vec, val_phase=True)
                    fwd01, back01 = self.denorm(fwd), self.denorm(back)
                    for i, ks in groups.items():
                        if len(ks) == len(ids):
                            meter.update(x01, back01, inm, i, j, "cycle")
                        else:
                            sel = torch.tensor(ks, dtype=torch.int64).pin_memory().to(self.device, non_blocking=True)
                            meter.update(x01.index_select(0, sel), back01.index_select(0, sel), [inm[k] for k in ks], i, j, "cycle")
                        if j in partner.get(i, ()):
                            for k in ks:
                                m, pid, z = inm[k].split("_")
                                translated.append((inm[k], f"{cfg.Modality(j).name}_{pid}_{z}", i, j, fwd01[k]))
            by_cell = {}
            for src, dst, i, j, t in translated:
                if dst in real:
                    by_cell.setdefault((i, j, tuple(t.shape)), []).append((src, t, real[dst]))
            for (i, j, _), items in by_cell.items():
                meter.update(torch.stack([t for _, t, _ in items]), torch.stack([r for _, _, r in items]),
                             [src for src, _, _ in items], i, j, "paired")
        tables = meter.result()
        log = translation_text(tables)
        maybe_mkdir(expr_root)
        with open(pjoin(expr_root, f"{self.modality}_translation_matrix.csv"), "w") as f:
            f.write(log)
        self.info(log)
        return tables
