#!/usr/bin/env python3
"""Calibration statistics (csrc/calibration.hip) at the test phase's batch, 16 x 256 x 256 x 5 logits and 15 bins: one
``ops.calibration_stats`` call against the same statistics composed from ATen ops on the same tensors, and one ``fit_temperature``
over 20 such batches.  Nothing is captured into a graph.

    python profiles/calibration_step.py                                   device-event timings, JSON
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/calibration_step.py --kernels
        the call alone, 40 times, a run of its own: which launches make it up
    python profiles/calibration_step.py --stats-csv DIR                   kernel times of such a run -> the finishing launch's share

Each call is timed on its own between two device events after warm-up calls; the figure is the median.  Bytes the algorithm needs:
4 C + 8 per pixel (logits once, int64 labels once); floor time = bytes / 8.0 TB/s (HBM specification; the batch sits in the
last-level cache, so the floor is a yardstick, not the expected bound)."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, S, C, BINS = 16, 256, 5, 15
HBM_PEAK = 8.0e12
KERNELS = ("k_calibration_finish", "k_calibration")        # (the longer name first: it contains the other)


def from_stats(path):
    rows = []
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    out = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        for k in KERNELS:
            if k in name and float(r.get("AverageNs") or 0.0) > 0:
                out.setdefault(k, {"calls": int(float(r.get("Calls", 0))), "avg_us": float(r["AverageNs"]) / 1e3,
                                   "min_us": float(r.get("MinNs") or 0.0) / 1e3})
                break
    if len(out) == 2:
        total = sum(v["avg_us"] for v in out.values())
        out["finish_share_of_kernel_time"] = out["k_calibration_finish"]["avg_us"] / total
        floor_us = (4 * C + 8) * N * S * S / HBM_PEAK * 1e6
        out["floor_us"], out["floor_over_main_kernel"] = floor_us, floor_us / out["k_calibration"]["avg_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--stats-csv", type=str, default=None)
    ap.add_argument("--calls", type=int, default=101)
    ap.add_argument("--fit-batches", type=int, default=20)
    args = ap.parse_args()
    if args.stats_csv:
        print(json.dumps({"shape": [N, S, S, C], "bins": BINS, "kernels": from_stats(args.stats_csv)}))
        return
    if args.calls < 31:
        raise SystemExit("the median needs at least 31 calls")

    import torch
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    from smsut_amd.misc import utils
    if not torch.cuda.is_available():
        raise SystemExit("profiles/calibration_step.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    gen = torch.Generator(device="cpu").manual_seed(5)

    def batch():
        z = (3.0 * torch.randn(N, S, S, C, generator=gen)).to(dev).permute(0, 3, 1, 2)        # logical NCHW, NHWC memory
        y = torch.randint(0, C, (N, S, S), generator=gen).to(dev)
        return z, y
    z, y = batch()
    lay = ops.CalibrationLayout(C, BINS)
    out = torch.zeros(lay.size, dtype=torch.float64, device=dev)
    ours = lambda: ops.calibration_stats(z, y, out, bins=BINS)
    if args.kernels:
        for _ in range(40):
            ours()
        torch.cuda.synchronize()
        return

    zr, yr = z.permute(0, 2, 3, 1).reshape(-1, C), y.reshape(-1)

    def aten():
        """the same totals from ATen ops (fp32 per pixel, fp64 sums), as one vector"""
        p = torch.softmax(zr, dim=1)
        conf, pred = p.max(dim=1)
        ok = (pred == yr).double()
        bins = (conf * float(BINS)).long().clamp_(max=BINS - 1)
        b3 = torch.stack([torch.bincount(bins, minlength=BINS).double(), torch.bincount(bins, weights=conf.double(), minlength=BINS),
                          torch.bincount(bins, weights=ok, minlength=BINS)], dim=1)
        nll = torch.logsumexp(zr, dim=1) - zr.gather(1, yr[:, None])[:, 0]
        brier = ((p - torch.nn.functional.one_hot(yr, C)) ** 2).sum(dim=1)
        c4 = torch.stack([torch.bincount(yr, minlength=C).double(), torch.bincount(yr, weights=ok, minlength=C),
                          torch.bincount(yr, weights=nll.double(), minlength=C),
                          torch.bincount(yr, weights=brier.double(), minlength=C)], dim=1)
        ez = (p * zr).sum(dim=1)
        g = (ez - zr.gather(1, yr[:, None])[:, 0]).double().sum()
        h = ((p * zr * zr).sum(dim=1) - ez * ez).clamp_(min=0).double().sum()
        return torch.cat([b3.reshape(-1), c4.reshape(-1), torch.stack([g, h]), torch.zeros(2, dtype=torch.float64, device=dev)])

    out.zero_()
    ours()
    a, b = out.clone(), aten()
    counts = torch.ones(lay.size, dtype=torch.bool)
    counts[1:3 * BINS:3] = False
    for k in range(C):
        counts[3 * BINS + 4 * k + 2:3 * BINS + 4 * k + 4] = False
    counts[lay.size - 4:lay.size - 2] = False
    same_counts = bool((a.cpu()[counts] == b.cpu()[counts]).all())
    rel = float(((a - b).abs() / b.abs().clamp(min=1.0)).max())
    assert rel < 1e-3, f"the ATen composition and the kernel disagree ({rel})"                 # before any timing

    def timed_each(fn, calls):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
        for st, en in ev:
            st.record()
            fn()
            en.record()
        torch.cuda.synchronize()
        return sorted(st.elapsed_time(en) * 1e3 for st, en in ev)       # us

    legs = {"kernel": ours, "aten": aten}
    for fn in legs.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    stat = {}
    for k, fn in legs.items():
        t = timed_each(fn, args.calls)
        stat[k] = {"median_us": t[len(t) // 2], "min_us": t[0], "p90_us": t[int(0.9 * len(t))], "calls": len(t)}

    batches = [(z, y)] + [batch() for _ in range(args.fit_batches - 1)]
    utils.fit_temperature(batches, C)                                  # warm-up
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fits = []
    for _ in range(5):
        st.record()
        t_fit, its = utils.fit_temperature(batches, C)
        en.record()
        torch.cuda.synchronize()
        fits.append(st.elapsed_time(en))
    fits.sort()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "shape": [N, S, S, C], "bins": BINS, "call": stat,
                      "aten_over_kernel": stat["aten"]["median_us"] / stat["kernel"]["median_us"],
                      "counts_equal_aten": same_counts, "largest_relative_difference_to_aten": rel,
                      "floor_us": (4 * C + 8) * N * S * S / HBM_PEAK * 1e6,
                      "fit": {"batches": len(batches), "iterations": its, "temperature": t_fit, "median_ms": fits[len(fits) // 2],
                              "all_ms": fits, "launches": 2 * len(batches) * its, "readbacks": its}}))


if __name__ == "__main__":
    main()
