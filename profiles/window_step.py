#!/usr/bin/env python3
"""Sliding-window inference: the fused blend (csrc/window.hip) against the same arithmetic composed from ATen ops, and one volume
end to end with the full field of view against the cropped one.

    python profiles/window_step.py                  # timings, one JSON line (device events, alternating, after warm-up)
    python profiles/window_step.py --lib OTHER.so   # the same with another build of the library (an A/B of two kernel forms)

(i)   ``ops.window_blend`` at 16 slices x 5 classes, window 256, overlap 0.5, on a 334 x 334 grid (2 x 2 tiles: a 512 x 512 scan at
      0.98 mm resampled to 1.5 mm) and on a 512 x 512 grid (3 x 3 tiles), prediction + confidence;
(ii)  the ATen composition on the same device tensors: a zeroed accumulator, one strided ``+=`` of ``w * p`` per tile, a division by
      the (precomputed) sum of the weights, ``max`` over the classes -- what an inference script built from torch would launch;
(iii) ``predict_volume`` of a (60, 334, 334) volume through the stock U-Net with ``field_of_view='full'`` and with ``'crop'``.
The comparison is always against (ii), never against the fused path itself.  Algorithmic bytes come from the shapes: per pixel
(tiles over it) * K * 4 in, 1 + 4 out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, K, WINDOW, OVERLAP = 16, 5, 256, 0.5
GRIDS = (334, 512)
HBM_PEAK = 8.0e12                 # bytes/s, MI355X HBM3E specification


def algorithmic_bytes(size, origins):
    cover = [sum(o <= i < o + WINDOW for o in origins) for i in range(size)]
    tiles_over_pixels = sum(cover) ** 2                        # the plan is the same on both axes: sum_y sum_x c(y) c(x)
    return N * (tiles_over_pixels * K * 4 + size * size * (1 + 4))


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
        raise SystemExit("profiles/window_step.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    wt = ops.window_weights(WINDOW, "gaussian", dev)
    wmap = (wt.view(-1, 1) * wt.view(1, -1)).view(1, WINDOW, WINDOW, 1)
    plans, tiles, wsum = {}, {}, {}
    for size in GRIDS:
        plans[size] = ops.window_plan(size, WINDOW, OVERLAP)
        n_tiles = len(plans[size]) ** 2
        tiles[size] = [torch.softmax(3 * torch.randn(N, WINDOW, WINDOW, K, generator=g), dim=-1).to(dev) for _ in range(n_tiles)]
        wsum[size] = torch.zeros(1, size, size, 1, device=dev)
        for y0 in plans[size]:
            for x0 in plans[size]:
                wsum[size][:, y0:y0 + WINDOW, x0:x0 + WINDOW] += wmap

    def fused(size):
        return lambda: ops.window_blend(tiles[size], plans[size], plans[size], (size, size), wt, wt, want_conf=True)

    def aten(size):
        def run():
            acc = torch.zeros(N, size, size, K, device=dev)
            it = iter(tiles[size])
            for y0 in plans[size]:
                for x0 in plans[size]:
                    acc[:, y0:y0 + WINDOW, x0:x0 + WINDOW] += wmap * next(it)
            conf, pred = (acc / wsum[size]).max(dim=-1)
            return pred.to(torch.uint8), conf
        return run

    check = {}
    for size in GRIDS:                                         # same arithmetic, before any timing
        (p, c, _), (rp, rc) = fused(size)(), aten(size)()
        check[size] = {"max_conf_diff": float((c - rc).abs().max()), "pred_mismatch": int((p != rp).sum())}
        assert check[size]["max_conf_diff"] < 1e-5 and check[size]["pred_mismatch"] <= 16, check

    def timed(fn, iters):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(iters):
            fn()
        en.record()
        torch.cuda.synchronize()
        return st.elapsed_time(en) / iters * 1e3               # us per call

    legs = {}
    for size in GRIDS:
        legs[f"blend{size}_fused"], legs[f"blend{size}_aten"] = fused(size), aten(size)
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                               # alternating
        for k, fn in legs.items():
            times[k].append(timed(fn, args.iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = {"device": torch.cuda.get_device_name(0), "lib": args.lib or "in-tree",
           "shape": {"slices": N, "K": K, "window": WINDOW, "overlap": OVERLAP}, "us_median": med, "us_all": times,
           "check_vs_aten": check}
    for size in GRIDS:
        b = algorithmic_bytes(size, plans[size])
        rate = b / (med[f"blend{size}_fused"] * 1e-6)
        out[f"blend{size}"] = {"tiles": len(plans[size]) ** 2, "algorithmic_MB": b / 1e6, "GB_per_s": rate / 1e9,
                               "share_of_hbm_peak": rate / HBM_PEAK,
                               "speedup_vs_aten": med[f"blend{size}_aten"] / med[f"blend{size}_fused"]}

    if not args.skip_volume:
        from smsut_amd.network.unet import UNet
        from smsut_amd.predict import Predictor, predict_volume
        torch.manual_seed(cfg.seed)
        net = UNet(cfg.img_channels, cfg.n_label + 1, cfg.base_width, norm_type="instance", act_type="lrelu").to(dev).eval()
        vol = (np.random.default_rng(2).standard_normal((60, 334, 334)) * 300.0).astype(np.float32)
        spacing = (5.0, 1.5, 1.5)                               # the resampled grid is the input's: 60 x 334 x 334
        p = Predictor(net, tta="none")
        vt = {}
        for fov in ("crop", "full"):
            run = lambda: predict_volume(p, vol, spacing, "ct", confidence=True, field_of_view=fov)
            res = run()
            torch.cuda.synchronize()
            vt[fov] = [timed(run, 3) / 1e3 for _ in range(3)]   # ms per volume, upload and cleanup included
            out[f"volume_{fov}_processed_shape"] = list(res.labels_processed.shape)
        out["predict_volume_ms"] = {k: sorted(v)[1] for k, v in vt.items()}
        out["predict_volume_ms_all"] = vt
    print(json.dumps(out))


if __name__ == "__main__":
    main()
