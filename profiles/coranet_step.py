#!/usr/bin/env python3
"""CoraNet loss head and step: the fused kernels (csrc/coranet.hip) against the same arithmetic composed from ATen ops.

    python profiles/coranet_step.py                     # timings, one JSON line (device events, alternating, after warm-up)
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/coranet_step.py --kernels-only     # a run of its own
    python profiles/coranet_step.py --stats-csv DIR     # kernel times of that run -> bytes/s and share of the HBM peak

(i)   fused loss head, forward + backward, at 8 + 8 slices of 256 x 256, L = 4 (13 channels);
(ii)  the ATen composition on the same device tensors: the three head cats, F.cross_entropy (weighted / per pixel), softmax,
      one-hot Dice, masked sums -- what the reference launches (trainer/coraNetTrainer.py:288-347);
(iii) the whole ``coraNetTrainer.train_iteration`` with (i) and with (ii).
The comparison is always against (ii), never against the fused path itself.  Algorithmic bytes come from the shapes."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, L, SIZE = 8, 4, 256
C = 3 * L + 1
HBM_PEAK = 8.0e12                 # bytes/s, MI355X HBM3E specification
# bytes per pixel each pass must move: logits (C fp32) in, labels int64, mask fp32, gradient (C fp32) out
BYTES = {"k_cora_sup_partial": 4 * C + 8, "k_cora_sup_bwd": 4 * C + 8 + 4 * C,
         "k_cora_semi_partial": 2 * 4 * C + 8 + 4, "k_cora_semi_bwd": 2 * 4 * C + 8 + 4 + 4 * C}


def algorithmic_bytes():
    px = N * SIZE * SIZE
    per = {k: v * px for k, v in BYTES.items()}
    return {"per_pixel": BYTES, "per_pass": per, "per_iteration": sum(per.values())}


def from_stats(path):
    rows = []
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    px = N * SIZE * SIZE
    out = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        for k, b in BYTES.items():
            if k in name:
                avg_ns, min_ns = float(r.get("AverageNs") or 0.0), float(r.get("MinNs") or 0.0)
                if avg_ns > 0:
                    rate = b * px / (avg_ns * 1e-9)
                    out[k] = {"avg_us": avg_ns / 1e3, "min_us": min_ns / 1e3, "calls": int(float(r.get("Calls", 0))),
                              "algorithmic_MB": b * px / 1e6, "GB_per_s": rate / 1e9, "share_of_hbm_peak": rate / HBM_PEAK}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--stats-csv", type=str, default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.stats_csv:
        print(json.dumps({"bytes": algorithmic_bytes(), "kernels": from_stats(args.stats_csv)}))
        return

    import torch
    import torch.nn.functional as F
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg, ops
    if not torch.cuda.is_available():
        raise SystemExit("profiles/coranet_step.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)

    def logits():
        return (2 * torch.randn(N, C, SIZE, SIZE, generator=g)).to(dev).contiguous(memory_format=torch.channels_last)
    z_sup, z_semi, e = logits().requires_grad_(True), logits().requires_grad_(True), logits()
    y = torch.randint(0, L + 1, (N, SIZE, SIZE), generator=g).to(dev)
    q = torch.randint(0, L + 1, (N, SIZE, SIZE), generator=g).to(dev)
    m = (torch.rand(N, SIZE, SIZE, generator=g) < 0.6).float().to(dev)
    wc = torch.tensor(cfg.class_weights(cfg.w_con, L), device=dev)
    wr = torch.tensor(cfg.class_weights(cfg.w_rad, L), device=dev)
    cw = 0.7

    # ---- (ii): the ATen composition
    def heads(z):
        return [torch.cat([z[:, :1], z[:, 1 + k * L:1 + (k + 1) * L]], dim=1) for k in range(3)]

    def dice(x, lab, batch):
        p = torch.softmax(x, dim=1)
        hot = torch.zeros_like(p).scatter_(1, lab.unsqueeze(1), 1.0)
        dims = (0, 2, 3) if batch else (2, 3)
        tp, fp, fn = (p * hot).sum(dims), (p * (1 - hot)).sum(dims), ((1 - p) * hot).sum(dims)
        dc = (2 * tp + 1e-5) / (2 * tp + fp + fn + 1e-5 + 1e-8)
        return 1.0 - (dc[1:] if batch else dc[:, 1:]).mean()

    def aten_sup(z, lab, w_con, w_rad, weight_ce, weight_dc, group=None):
        h0, h1, h2 = heads(z)
        cedc = weight_dc * dice(h0, lab, True) + weight_ce * F.cross_entropy(h0, lab)
        con, rad = F.cross_entropy(h1, lab, weight=w_con), F.cross_entropy(h2, lab, weight=w_rad)
        return torch.stack([(cedc + con + rad) / 4, cedc, con, rad])

    def aten_semi(z, te, plab, mask, w):
        hz, he = heads(z), heads(te.detach())
        certain = ((F.cross_entropy(hz[0], plab, reduction="none") * mask).sum() / (mask.sum() + 1e-16) + dice(hz[0], plab, False)) / 2
        um = (1 - mask).unsqueeze(1)
        unc = sum(w * (((torch.softmax(a, 1) - torch.softmax(b, 1)) ** 2 * um).sum() / (um.sum() + 1e-16)) for a, b in zip(hz, he)) / 3
        return torch.stack([certain, unc])

    def head(sup_fn, semi_fn):
        z_sup.grad = z_semi.grad = None
        s = sup_fn(z_sup, y, wc, wr, 0.5, 0.5)
        t = semi_fn(z_semi, e, q, m, cw)
        (s[0] + t[0] + 0.1 * t[1]).backward()
        return torch.cat([s.detach(), t.detach()])

    fused_head = lambda: head(ops.cora_sup_loss, ops.cora_semi_loss)
    aten_head = lambda: head(aten_sup, aten_semi)

    if args.kernels_only:
        for _ in range(20):
            fused_head()
        torch.cuda.synchronize()
        return

    a, b = fused_head().tolist(), aten_head().tolist()
    assert all(abs(x - r) <= 1e-4 * abs(r) + 1e-6 for x, r in zip(a, b)), (a, b)         # same arithmetic, before any timing

    # ---- (iii): the trainer's step with either head
    import types
    from smsut_amd.trainer.coraNetTrainer import coraNetTrainer
    torch.manual_seed(cfg.seed)
    tr = coraNetTrainer("train", types.SimpleNamespace(fold=0, expr_name=None, write_env=False, model_id=None))
    tr.net.train(); tr.ema.train()
    tr.epoch, tr.iter = 20, 1200
    img1 = (0.5 * torch.randn(N, 1, SIZE, SIZE, generator=g)).clamp_(-1, 1).to(dev)
    img2 = (0.5 * torch.randn(N, 1, SIZE, SIZE, generator=g)).clamp_(-1, 1).to(dev)
    with torch.no_grad():
        pq, pm = ops.cora_pseudo(tr.net(img2))
    fused_fns = (ops.cora_sup_loss, ops.cora_semi_loss)

    def step(fns):
        ops.cora_sup_loss, ops.cora_semi_loss = fns
        try:
            return tr.train_iteration(img1, y, img2, pq, pm)
        finally:
            ops.cora_sup_loss, ops.cora_semi_loss = fused_fns

    def timed(fn, iters):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(iters):
            fn()
        en.record()
        torch.cuda.synchronize()
        return st.elapsed_time(en) / iters * 1e3            # us per call

    legs = {"head_fused": fused_head, "head_aten": aten_head,
            "step_fused": lambda: step(fused_fns), "step_aten": lambda: step((aten_sup, aten_semi))}
    for fn in legs.values():                                 # warm-up of every shape the timed windows use
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                             # alternating
        for k, fn in legs.items():
            times[k].append(timed(fn, args.iters if k.startswith("head") else max(args.iters // 2, 5)))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({"device": torch.cuda.get_device_name(0), "shape": {"slices": [N, N], "size": SIZE, "L": L},
                      "us_median": med, "us_all": times,
                      "head_speedup_vs_aten": med["head_aten"] / med["head_fused"],
                      "step_speedup_vs_aten": med["step_aten"] / med["step_fused"], "bytes": algorithmic_bytes()}))


if __name__ == "__main__":
    main()
