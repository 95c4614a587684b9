#!/usr/bin/env python3
"""``ops.image_similarity`` (csrc/similarity.hip: SSIM, SE, AE of two image batches in one pass) against the same arithmetic
composed from ATen ops, at 16 x 256 x 256 and 16 x 512 x 512.

    python profiles/translation_step.py                  # whole-call wall times, one JSON line
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/translation_step.py --kernels-only   # a run of its own
    python profiles/translation_step.py --stats-csv DIR  # the kernels' times in that run -> bytes/s and share of the HBM peak

Whole call: ``torch.cuda.synchronize()`` on both sides of ONE call, the two legs alternating in one process, ``--calls`` (>= 31)
timed calls each after a warm-up, medians reported with every sample kept.
(i)  fused   ``ops.image_similarity(a, b, 1.0)``: two launches (tiles, per-slice sum), fp64 [N, 3] left on the device;
(ii) aten    the five planes a, b, a^2, b^2, ab stacked as channels, one depthwise ``F.conv2d`` with the 11 x 11 window (groups = 5,
             no padding), the pointwise SSIM expression, and fp64 sums of the SSIM map, (a-b)^2 and |a-b| per slice.
Before any timing the two results are compared (SSIM sums to 1e-4 relative: the ATen leg sums its window in another order).
``--kernels-only`` runs the fused call alone at both shapes (the profiler's run); the kernel time is k_similarity_tiles'
average in that run, the algorithmic bytes 2 N H W 4 (each input read once; out and the partials are negligible)."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((16, 256, 256), (16, 512, 512))
HBM_PEAK = 8.0e12


def from_stats(path):
    """Per kernel name the stats rows of the run.  Both shapes ran in it with equal call counts, so a kernel's average is over
    both; the per-shape split needs the trace rows (``*kernel_trace.csv``), read here when present."""
    out = {}
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Name") or r.get("KernelName") or ""
            if "k_similarity" in name:
                key = "tiles" if "tiles" in name else "final"
                out[key] = {"calls": int(float(r.get("Calls", 0))), "avg_us": float(r.get("AverageNs") or 0.0) / 1e3,
                            "min_us": float(r.get("MinNs") or 0.0) / 1e3, "max_us": float(r.get("MaxNs") or 0.0) / 1e3}
    per_grid = {}
    for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name") or r.get("Name") or ""
            if "k_similarity_tiles" in name:
                grid = int(float(r.get("Grid_Size_X") or r.get("Grid_Size") or 0))
                per_grid.setdefault(grid, []).append(float(r["End_Timestamp"]) - float(r["Start_Timestamp"]))
    shapes = {}
    for (n, h, w), grid in zip(SHAPES, sorted(per_grid)):
        ns = sorted(per_grid[grid])[len(per_grid[grid]) // 2]
        b = 2 * n * h * w * 4
        shapes[f"{n}x{h}x{w}"] = {"calls": len(per_grid[grid]), "median_us": ns / 1e3, "min_us": min(per_grid[grid]) / 1e3,
                                  "algorithmic_MB": b / 1e6, "GB_per_s": b / ns, "share_of_hbm_peak": b / (ns * 1e-9) / HBM_PEAK}
    return {"stats": out, "k_similarity_tiles_by_shape": shapes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--stats-csv", type=str, default=None)
    ap.add_argument("--calls", type=int, default=41)
    args = ap.parse_args()
    if args.stats_csv:
        print(json.dumps(from_stats(args.stats_csv)))
        return

    import torch
    import torch.nn.functional as F
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("profiles/translation_step.py measures on the GPU; none is visible")
    assert args.calls >= 31
    k = torch.arange(-5, 6, dtype=torch.float64)
    w1 = torch.exp(-k * k / (2 * 1.5 ** 2))
    w1 /= w1.sum()
    win = torch.outer(w1, w1).to(torch.float32).cuda()[None, None].repeat(5, 1, 1, 1).contiguous()
    c1, c2 = 0.01 ** 2, 0.03 ** 2

    def aten(a, b):
        planes = torch.stack([a, b, a * a, b * b, a * b], 1)
        m = F.conv2d(planes, win, groups=5)
        mx, my, xx, yy, xy = m.unbind(1)
        sx, sy, sxy = xx - mx * mx, yy - my * my, xy - mx * my
        s = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sx + sy + c2))
        d = a.double() - b.double()
        return torch.stack([s.double().sum((1, 2)), (d * d).sum((1, 2)), d.abs().sum((1, 2))], 1)

    def fused(a, b):
        return ops.image_similarity(a, b, 1.0)

    def wall(fn, a, b):
        torch.cuda.synchronize()
        tic = time.perf_counter()
        out = fn(a, b)
        torch.cuda.synchronize()
        return time.perf_counter() - tic, out

    result = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "shapes": {}}
    for n, h, w in SHAPES:
        g = torch.Generator(device="cpu").manual_seed(5 + h)
        a = torch.rand(n, h, w, generator=g).cuda()
        b = (a + 0.05 * torch.randn(n, h, w, generator=g).cuda()).clamp_(0, 1)
        if args.kernels_only:
            for _ in range(args.calls):
                wall(fused, a, b)
            continue
        for _ in range(5):                                   # warm-up, and the comparison
            got, want = wall(fused, a, b)[1], wall(aten, a, b)[1]
        rel = ((got - want).abs() / want.abs()).max(0).values.tolist()
        assert rel[0] < 1e-4 and rel[1] < 1e-12 and rel[2] < 1e-12, rel
        assert torch.equal(got, fused(a, b))                 # bitwise from call to call
        t = {"fused": [], "aten": []}
        for _ in range(args.calls):                          # alternating
            t["fused"].append(wall(fused, a, b)[0])
            t["aten"].append(wall(aten, a, b)[0])
        med = {kk: sorted(v)[len(v) // 2] for kk, v in t.items()}
        result["shapes"][f"{n}x{h}x{w}"] = {"us_median": {kk: v * 1e6 for kk, v in med.items()}, "aten_over_fused": med["aten"] / med["fused"],
                                           "max_rel_diff": rel, "us_all": {kk: [round(x * 1e6, 1) for x in v] for kk, v in t.items()}}
    if not args.kernels_only:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
