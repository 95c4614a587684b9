#!/usr/bin/env python3
"""``data_pprocess.volume.prepare_volume`` (csrc/volume.hip) at a CHAOS-like MR volume (30, 256, 256) @ (7.7, 1.89, 1.89) mm ->
(46, 256, 256) and a BTCV-like CT volume (120, 512, 512) @ (3.0, 0.8, 0.8) mm -> (72, 256, 256), against scipy on the host.

    python profiles/volume_step.py                       # whole-call wall times, one JSON line
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/volume_step.py --kernels-only --shape chaos   # own run
    python profiles/volume_step.py --trace-csv DIR --shape chaos     # the kernels' times in that run -> bytes/s, share of HBM peak

Whole call: ``torch.cuda.synchronize()`` on both sides of ONE ``prepare_volume`` call on device-resident inputs (image fp32, label
uint8), ``--calls`` timed calls after a warm-up, the median reported and every sample kept; ``upload`` is the same call on NumPy
inputs (host-to-device copies included).  Host leg, ``--cpu-calls`` times: ``scipy.ndimage.spline_filter(order=3, mode='mirror')``,
``map_coordinates(order=3, prefilter=False)`` on the window's grid, ``map_coordinates(order=0)`` for the label, ``np.percentile`` or
the CT bounds, and the window expression; when scipy is missing, tests/volume_ref.py's oracle.  The two legs' 8-bit images are
compared first (share of differing bytes; the host leg interpolates in fp64).
Kernel times: every launch of the profiler's run by name, in launch order (the strided prefilter runs twice a call: y, then z);
algorithmic bytes are each kernel's input read once plus its output written once."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {"chaos": ((30, 256, 256), (7.7, 1.89, 1.89), "t2"), "btcv": ((120, 512, 512), (3.0, 0.8, 0.8), "ct")}
HBM_PEAK = 8.0e12


def kernel_bytes(old, out):
    n, m = old[0] * old[1] * old[2], out[0] * out[1] * out[2]
    return {"bsp_filter_x": 8 * n, "bsp_filter_s": 8 * n, "resample_cubic": 4 * n + 4 * m, "resample_nearest": n + m,
            "os_hist": 4 * m, "window_u8": 5 * m}


def from_trace(path, shape):
    from smsut_amd.data_pprocess import volume as V
    old, sp, _ = SHAPES[shape]
    nbytes = kernel_bytes(old, V.resample_plan(old, sp).out_size)
    rows = []
    for f in glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((float(r["Start_Timestamp"]), r.get("Kernel_Name") or r.get("Name") or "",
                         float(r["End_Timestamp"]) - float(r["Start_Timestamp"])))
    rows.sort()
    per, seen_s = {}, 0
    for _, name, ns in rows:
        key = next((k for k in nbytes if k in name), None)
        if key is None:
            continue
        label = key
        if key == "bsp_filter_s":
            label = "bsp_filter_s[%s]" % ("y" if seen_s % 2 == 0 else "z")
            seen_s += 1
        per.setdefault(label, (key, []))[1].append(ns)
    out = {}
    for label, (key, v) in per.items():
        med = sorted(v)[len(v) // 2]
        out[label] = {"launches": len(v), "median_us": med / 1e3, "min_us": min(v) / 1e3, "algorithmic_MB": nbytes[key] / 1e6,
                      "GB_per_s": nbytes[key] / med, "share_of_hbm_peak": nbytes[key] / (med * 1e-9) / HBM_PEAK}
    return out


def host_leg(img, raw, plan, modality):
    import numpy as np
    import volume_ref as R
    old = img.shape
    grid = np.meshgrid(*(R.coords(plan.out_size[a], plan.start[a], old[a], plan.new_size[a]) for a in range(3)), indexing="ij")
    ok = np.logical_and.reduce([R.inside(g, old[a]) for a, g in enumerate(grid)])
    try:
        from scipy import ndimage as ndi
        coef = ndi.spline_filter(img.astype(np.float64), order=3, mode="mirror")
        vol = np.where(ok, ndi.map_coordinates(coef, grid, order=3, mode="mirror", prefilter=False), 0.0)
        how = "scipy"
    except ImportError:
        vol = R.resample(R.coefficients(img), plan.out_size, old, plan.new_size, plan.start)[0]
        how = "oracle"
    lab = R.nearest(raw, plan.out_size, old, plan.new_size, plan.start)
    vol = vol.astype(np.float32)
    if modality == "ct":
        lo, hi = max(float(vol.min()), -1000.0), min(float(vol.max()), 400.0)
    else:
        lo, hi = np.percentile(vol.astype(np.float64), [0.05, 99.5])
    return R.window(vol, lo, hi, np.float32), lab, how


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--trace-csv", type=str, default=None)
    ap.add_argument("--shape", choices=list(SHAPES), default=None)
    ap.add_argument("--calls", type=int, default=31)
    ap.add_argument("--cpu-calls", type=int, default=3)
    args = ap.parse_args()
    import smsut_amd  # noqa: F401
    if args.trace_csv:
        print(json.dumps({args.shape: from_trace(args.trace_csv, args.shape)}))
        return

    import numpy as np
    import torch
    import volume_ref as R
    from smsut_amd.data_pprocess import volume as V
    if not torch.cuda.is_available():
        raise SystemExit("profiles/volume_step.py measures on the GPU; none is visible")

    def wall(fn):
        torch.cuda.synchronize()
        tic = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - tic, out

    result = {"device": torch.cuda.get_device_name(0), "calls": args.calls, "cpu_calls": args.cpu_calls, "shapes": {}}
    for name in ([args.shape] if args.shape else list(SHAPES)):
        old, sp, modality = SHAPES[name]
        img = R.volume(old, 7) - (1024.0 if modality == "ct" else 0.0)
        raw = R.blocky_labels(old, 8, block=16)
        dimg, draw = torch.from_numpy(img).cuda(), torch.from_numpy(raw).cuda()
        for _ in range(5):
            image_u8, label_u8, plan = V.prepare_volume(dimg, draw, sp, modality)
        if args.kernels_only:
            for _ in range(args.calls):
                wall(lambda: V.prepare_volume(dimg, draw, sp, modality))
            continue
        t_dev = [wall(lambda: V.prepare_volume(dimg, draw, sp, modality))[0] for _ in range(args.calls)]
        t_up = [wall(lambda: V.prepare_volume(img, raw, sp, modality))[0] for _ in range(args.calls)]
        t_cpu = []
        for _ in range(args.cpu_calls):
            tic = time.perf_counter()
            himg, hlab, how = host_leg(img, raw, plan, modality)
            t_cpu.append(time.perf_counter() - tic)
        got = image_u8.cpu().numpy()
        diff = got.astype(np.int16) - himg.astype(np.int16)
        med = lambda v: sorted(v)[len(v) // 2]                                   # noqa: E731
        result["shapes"][name] = {
            "in": old, "out": plan.out_size, "new_size": plan.new_size, "modality": modality, "host_leg": how,
            "ms_median": {"device_inputs": med(t_dev) * 1e3, "upload": med(t_up) * 1e3, "host": med(t_cpu) * 1e3},
            "host_over_device": med(t_cpu) / med(t_dev),
            "image_bytes_differing": float((diff != 0).mean()), "image_max_level_diff": int(np.abs(diff).max()),
            "labels_equal": bool(np.array_equal(label_u8.cpu().numpy(), hlab)),
            "ms_all": {"device_inputs": [round(x * 1e3, 3) for x in t_dev], "upload": [round(x * 1e3, 3) for x in t_up],
                       "host": [round(x * 1e3, 1) for x in t_cpu]}}
    if not args.kernels_only:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
