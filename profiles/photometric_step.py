#!/usr/bin/env python3
"""Photometric augmentation (csrc/photometric.hip) at the loader's batch: kernel times against their byte floor, and the same
chain composed from ATen ops.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/photometric_step.py --loader --size 256
        a short InTurnLoader loop (16 slices per batch, colorJitter + gammaCorrect on, mostly-black slices); a run of its own
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/photometric_step.py --kernels --content random --size 256
        the two kernels alone on full-range noise (--content sparse: >= 90 % zeros), to compare the histogram's two regimes
    python profiles/photometric_step.py --stats-csv DIR --size 256        kernel times of such a run -> share of the byte floor
    python profiles/photometric_step.py --size 256                        device-event timings against the ATen composition, JSON

Byte floor: the histogram pass must read 4 B/pixel, the apply pass read 4 and write 4; floor time = bytes / 8.0 TB/s (HBM
specification; at these sizes the batch sits in the last-level cache, so the floor is a yardstick, not the expected bound)."""
import argparse
import csv
import glob
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 16
HBM_PEAK = 8.0e12
BYTES = {"k_photo_hist": 4, "k_photo_apply": 8}


def from_stats(path, size):
    rows = []
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    px = N * size * size
    out = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        for k, b in BYTES.items():
            if k in name and float(r.get("AverageNs") or 0.0) > 0:
                avg_ns, min_ns = float(r["AverageNs"]), float(r.get("MinNs") or 0.0)
                floor_ns = b * px / HBM_PEAK * 1e9
                out[k] = {"calls": int(float(r.get("Calls", 0))), "avg_us": avg_ns / 1e3, "min_us": min_ns / 1e3,
                          "algorithmic_MB": b * px / 1e6, "floor_us": floor_ns / 1e3, "floor_over_avg": floor_ns / avg_ns}
    return out


def slices(n, size, content, seed=0):
    """uint8 [n, size, size]: 'random' = full-range noise; 'sparse' = black with a textured disc covering < 10 % (an MR / CT slice's
    background-to-body ratio is milder; this is the worst case for same-address adds)."""
    import numpy as np
    rs = np.random.RandomState(seed)
    img = rs.randint(0, 256, (n, size, size)).astype(np.uint8)
    if content == "sparse":
        yy, xx = np.mgrid[0:size, 0:size]
        img[:, (yy - size // 2) ** 2 + (xx - size // 2) ** 2 > (0.17 * size) ** 2] = 0
        assert (img == 0).mean() >= 0.9
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--loader", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--content", choices=("random", "sparse"), default="sparse")
    ap.add_argument("--stats-csv", type=str, default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.stats_csv:
        print(json.dumps({"size": args.size, "slices": N, "kernels": from_stats(args.stats_csv, args.size)}))
        return

    import numpy as np
    import torch
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    from smsut_amd.data_loader import gpu_augment as ga, inTurnLoader as inlod
    if not torch.cuda.is_available():
        raise SystemExit("profiles/photometric_step.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    S = args.size
    flags = dict(cfg.data_aug, rotate=False, elasticDeform=False, resizeCrop=False, colorJitter=True, gammaCorrect=True)
    photo = ga.GpuPhotometricAugment(flags)
    random.seed(1)

    if args.loader:
        class DS:
            images = torch.from_numpy(slices(4 * N, S, "sparse"))
            labels = torch.zeros(4 * N, S, S, dtype=torch.uint8)
            modality = [0] * (4 * N)
            names = [f"m_{i:03d}_000" for i in range(4 * N)]
        sampler = inlod.InTurnTestBatchSampler([list(range(4 * N))], N)
        for _ in range(6):                                   # 24 batches
            for _batch in inlod.InTurnLoader(DS, sampler, dev, None, photo):
                pass
        torch.cuda.synchronize()
        return

    x = torch.from_numpy(slices(N, S, args.content)).to(dev).float().div_(255.0).unsqueeze(1)
    jit, gam = photo.draw(N)
    if args.kernels:
        for _ in range(24):
            ga.photometric(x, jit, gam, normalize=True)
        torch.cuda.synchronize()
        return

    # ---- the same chain from ATen ops: quantise, bincount, table build on [N, 256], gather
    order = torch.tensor([[j[0]] for j in jit], device=dev)
    b = torch.tensor([[j[1]] for j in jit], dtype=torch.float32, device=dev)
    c = torch.tensor([[j[2]] for j in jit], dtype=torch.float32, device=dev)
    gtab = torch.from_numpy(np.stack([np.arange(256, dtype=np.uint8) if g is None else ga.gamma_table(g) for g in gam])).to(dev).long()
    out_tab = ga.level_table(dev, True)
    offs = (torch.arange(N, device=dev) * 256).unsqueeze(1)
    ident = torch.arange(256, device=dev, dtype=torch.float32).expand(N, 256)

    def blend(d, v, a):
        return (d + a * (v - d)).clamp_(0.0, 255.0).trunc_()

    def aten_chain(img):
        lv = (img * 255.0).add_(0.5).floor_().clamp_(0.0, 255.0).long().view(N, -1)
        hist = torch.bincount((lv + offs).view(-1), minlength=N * 256).view(N, 256).double()

        def mean(cur):
            return ((hist * cur.double()).sum(1, keepdim=True) / float(S * S) + 0.5).floor_().float()
        br = blend(0.0, ident, b)
        bc = blend(mean(br), br, c)
        cb = blend(0.0, blend(mean(ident), ident, c), b)
        cur = torch.where(order == 0, bc, cb).long()
        tab = out_tab[gtab.gather(1, cur)]
        return tab.gather(1, lv).view_as(img)

    ours = lambda: ga.photometric(x, jit, gam, normalize=True)
    aten = lambda: aten_chain(x)
    assert torch.equal(ours(), aten()), "the ATen composition and the kernels disagree"        # same bits, before any timing

    def timed(fn, iters):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(iters):
            fn()
        en.record()
        torch.cuda.synchronize()
        return st.elapsed_time(en) / iters * 1e3            # us per call

    legs = {"kernels": ours, "aten": aten}
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                             # alternating
        for k, fn in legs.items():
            times[k].append(timed(fn, args.iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({"device": torch.cuda.get_device_name(0), "slices": N, "size": S, "content": args.content,
                      "us_median": med, "us_all": times, "aten_over_kernels": med["aten"] / med["kernels"]}))


if __name__ == "__main__":
    main()
