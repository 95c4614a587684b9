#!/usr/bin/env python3
"""Dual-task consistency: the signed-distance-map launches, the fused loss and the whole step (csrc/dtc.hip).

    python profiles/dtc_step.py                         # timings, one JSON line (device events, alternating, after warm-up)

At 8 + 8 slices of 256 x 256, C = 5, on one GPU:
(i)   ``ops.signed_distance_map`` alone (three launches) on labels as the synthetic loader draws them, on the worst input for the
      column search (one member pixel in a corner: every search spans its column), and on background-only slices (full / empty images);
(ii)  ``ops.dtc_loss`` forward + backward against the same arithmetic composed from ATen ops on the same device tensors;
(iii) the network's forward pass alone, and the whole ``dtcTrainer.train_iteration`` with (ii) fused and composed;
(iv)  the host route, if scipy is importable here: ``scipy.ndimage.distance_transform_edt`` twice per (slice, class) pair.
The comparison of (ii) is always against the ATen composition, never against the fused path itself."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C, SIZE, K = 8, 5, 256, 1500.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()

    import types
    import numpy as np
    import torch
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg, ops
    from smsut_amd.misc.synthetic import SyntheticSliceLoader
    if not torch.cuda.is_available():
        raise SystemExit("profiles/dtc_step.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    assert cfg.n_label + 1 == C and cfg.input_size == SIZE and cfg.batch_size == N

    _, msk, _, _ = next(iter(SyntheticSliceLoader(N, n_batches=1, device=dev, labeled=True, rank=0)))
    msk = msk.to(dev)
    corner = torch.zeros_like(msk)
    corner[:, -1, -1] = C - 1
    background = torch.zeros_like(msk)                      # background-only slices: one full and C - 1 empty images each

    def rnd(*shape):
        return torch.randn(*shape, generator=g)
    half = (torch.rand(2 * N, C, SIZE, SIZE, generator=g) < 0.5)
    t0 = torch.where(half, (torch.rand(2 * N, C, SIZE, SIZE, generator=g) - 0.5) * 1e-2, torch.rand(2 * N, C, SIZE, SIZE, generator=g) * 2 - 1)
    t = t0.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    z = (2 * rnd(2 * N, C, SIZE, SIZE)).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    sdf = ops.signed_distance_map(msk, C)

    def aten_loss(tt, zz, ss, k=K):
        b = ss.shape[0]
        return torch.stack([((tt[:b] - ss) ** 2).mean(), ((torch.sigmoid(-k * tt) - torch.softmax(zz, dim=1)) ** 2).mean()])

    def head(fn):
        t.grad = z.grad = None
        out = fn(t, z, sdf, K)
        (0.3 * out[0] + 0.3 * out[1]).backward()
        return out.detach()

    a, b = head(ops.dtc_loss).tolist(), head(aten_loss).tolist()
    assert all(abs(x - r) <= 1e-4 * abs(r) + 1e-6 for x, r in zip(a, b)), (a, b)           # same arithmetic, before any timing

    from smsut_amd.trainer.dtcTrainer import dtcTrainer
    torch.manual_seed(cfg.seed)
    tr = dtcTrainer("train", types.SimpleNamespace(fold=0, expr_name=None, write_env=False, model_id=None))
    tr.net.train()
    tr.epoch, tr.iter = 20, 1200
    img = (0.5 * rnd(2 * N, 1, SIZE, SIZE)).clamp_(-1, 1).to(dev)
    fused = ops.dtc_loss

    def step(fn):
        ops.dtc_loss = fn
        try:
            return tr.train_iteration(img, msk)
        finally:
            ops.dtc_loss = fused

    def net_fwd():
        with torch.no_grad(), ops.wino_prepared(tr.net, forms="f"):
            return tr.net(img)

    def timed(fn, iters):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(iters):
            fn()
        en.record()
        torch.cuda.synchronize()
        return st.elapsed_time(en) / iters * 1e3            # us per call

    legs = {"sdf_synthetic": lambda: ops.signed_distance_map(msk, C), "sdf_corner": lambda: ops.signed_distance_map(corner, C),
            "sdf_background": lambda: ops.signed_distance_map(background, C),
            "loss_fused": lambda: head(ops.dtc_loss), "loss_aten": lambda: head(aten_loss), "net_forward": net_fwd,
            "step_fused": lambda: step(fused), "step_aten": lambda: step(aten_loss)}
    for fn in legs.values():                                 # warm-up of every shape the timed windows use
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                             # alternating
        for k, fn in legs.items():
            times[k].append(timed(fn, args.iters if not k.startswith(("step", "net")) else max(args.iters // 2, 5)))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}

    host = None
    try:
        from scipy import ndimage
        lab = msk.cpu().numpy()
        pairs = [(lab[i] == c) for i in range(N) for c in range(C)]
        tic = time.perf_counter()
        for p in pairs:
            ndimage.distance_transform_edt(p); ndimage.distance_transform_edt(~p)
        host = {"ms_per_pair": (time.perf_counter() - tic) / len(pairs) * 1e3, "pairs": len(pairs)}
    except ImportError:
        pass
    px = N * C * SIZE * SIZE
    print(json.dumps({"device": torch.cuda.get_device_name(0), "shape": {"slices": [N, N], "size": SIZE, "C": C},
                      "us_median": med, "us_all": times, "loss_speedup_vs_aten": med["loss_aten"] / med["loss_fused"],
                      "step_speedup_vs_aten": med["step_aten"] / med["step_fused"], "scipy_host": host,
                      "sdf_bytes": {"labels": 8 * N * SIZE * SIZE, "d2_write_read": 8 * px, "sdf_write": 4 * px},
                      "members_share": float((msk > 0).float().mean())}))


if __name__ == "__main__":
    main()
