#!/usr/bin/env python3
"""Test-time augmentation: the fused merge (csrc/tta.hip) against the same arithmetic composed from ATen ops, and one volume end
to end.

    python profiles/tta_step.py                     # timings, one JSON line (device events, alternating, after warm-up)
    python profiles/tta_step.py --lib OTHER.so      # the same with another build of the library (the tile A/B: a library compiled
                                                    # with -DSMSUT_TTA_TILE32_MAXC=0 runs 16 x 16 tiles everywhere)

(i)   ``ops.tta_merge`` at 8 members x 16 slices x 256 x 256 x 5 channels, and at 4 members ('flips'), prediction + confidence;
(ii)  the ATen composition on the same device tensors: softmax per member, inverse flip / rot90, stack, mean, max -- what an
      inference script built from torch would launch;
(iii) ``predict_volume`` of a (30, 256, 256) volume through the stock U-Net with 'none', 'flips' and 'd4'.
The comparison is always against (ii), never against the fused path itself.  Algorithmic bytes come from the shapes:
T * C * 4 in, 1 + 4 out per pixel."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, SIZE, C = 16, 256, 5
HBM_PEAK = 8.0e12                 # bytes/s, MI355X HBM3E specification


def algorithmic_bytes(t):
    return N * SIZE * SIZE * (t * C * 4 + 1 + 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", type=str, default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-volume", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip, config as cfg, ops
    if args.lib:
        _hip.LIB_PATH = os.path.abspath(args.lib)
    if not torch.cuda.is_available():
        raise SystemExit("profiles/tta_step.py measures on the GPU; none is visible")
    import tta_ref as R
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    sets = {8: ops.tta_transforms("d4"), 4: ops.tta_transforms("flips")}
    members = [(3 * torch.randn(N, SIZE, SIZE, C, generator=g)).to(dev).permute(0, 3, 1, 2) for _ in range(8)]

    def fused(t):
        return lambda: ops.tta_merge(members[:t], sets[t], want_conf=True)

    def aten(t):
        def run():
            ps = [R.inv(torch.softmax(z, dim=1), gg) for z, gg in zip(members[:t], sets[t])]
            conf, pred = torch.stack(ps).mean(0).max(dim=1)
            return pred.to(torch.uint8), conf
        return run

    check = {}
    for t in (8, 4):                                           # same arithmetic, before any timing
        (p, c, _), (rp, rc) = fused(t)(), aten(t)()
        check[t] = {"max_conf_diff": float((c - rc).abs().max()), "pred_mismatch": int((p != rp).sum())}
        assert check[t]["max_conf_diff"] < 1e-5 and check[t]["pred_mismatch"] <= 16, check

    def timed(fn, iters):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(iters):
            fn()
        en.record()
        torch.cuda.synchronize()
        return st.elapsed_time(en) / iters * 1e3               # us per call

    legs = {"merge8_fused": fused(8), "merge8_aten": aten(8), "merge4_fused": fused(4), "merge4_aten": aten(4)}
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                               # alternating
        for k, fn in legs.items():
            times[k].append(timed(fn, args.iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = {"device": torch.cuda.get_device_name(0), "lib": args.lib or "in-tree", "shape": {"slices": N, "size": SIZE, "C": C},
           "us_median": med, "us_all": times, "check_vs_aten": check}
    for t in (8, 4):
        b = algorithmic_bytes(t)
        rate = b / (med[f"merge{t}_fused"] * 1e-6)
        out[f"merge{t}"] = {"algorithmic_MB": b / 1e6, "GB_per_s": rate / 1e9, "share_of_hbm_peak": rate / HBM_PEAK,
                            "speedup_vs_aten": med[f"merge{t}_aten"] / med[f"merge{t}_fused"]}

    if not args.skip_volume:
        from smsut_amd.network.unet import UNet
        from smsut_amd.predict import Predictor, predict_volume
        torch.manual_seed(cfg.seed)
        net = UNet(cfg.img_channels, cfg.n_label + 1, cfg.base_width, norm_type="instance", act_type="lrelu").to(dev).eval()
        vol = (np.random.default_rng(2).standard_normal((30, SIZE, SIZE)) * 300.0).astype(np.float32)
        spacing = (5.0, 1.5, 1.5)
        vt = {}
        for tta in ("none", "flips", "d4"):
            p = Predictor(net, tta=tta)
            run = lambda: predict_volume(p, vol, spacing, "ct", confidence=(tta != "none"))
            run()
            torch.cuda.synchronize()
            vt[tta] = [timed(run, 3) / 1e3 for _ in range(3)]   # ms per volume, upload and cleanup included
        out["predict_volume_ms"] = {k: sorted(v)[1] for k, v in vt.items()}
        out["predict_volume_ms_all"] = vt
    print(json.dumps(out))


if __name__ == "__main__":
    main()
