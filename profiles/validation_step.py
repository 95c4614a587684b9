#!/usr/bin/env python3
"""One whole validation pass, on the host (the path every trainer takes with ``config.validate_on_device`` off) and on the device
(csrc/evaluate.hip, ``BaseTrainer.validate_epoch_device``).

    python profiles/validation_step.py                  # wall times, one JSON line
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/validation_step.py --kernels-only    # a run of its own
    python profiles/validation_step.py --stats-csv DIR  # k_eval_overlap's time in that run -> bytes/s and share of the HBM peak

One ``UnetTrainer`` with random weights validates the synthetic loader at 256 x 256: 80 batches of 8 slices = 80 volumes, 640 slices,
5 classes.  Each leg is the wall time of the whole pass with ``torch.cuda.synchronize()`` on both sides, the loader rewound to the
same generator state first; one warm-up round, then ``--rounds`` rounds alternating the legs, medians reported:
(i)   host    ``_collect_labels`` + ``validate_epoch`` + ``validate_dice`` -- the label pass over the loader, ``loss.item()`` and the
              int64 argmax copied to the host per batch, NumPy Dice;
(ii)  device  ``validate_epoch_device`` + ``validate_dice_device`` -- nothing read back until the loader is exhausted;
(iii) forward the same batches through the network alone (what is left once validation itself costs nothing);
(iv)  loader  the loader alone (the synthetic source draws its batches on the CPU; (i) walks it twice, the others once).
Before any timing the two Dice dicts and the two meters are compared: they must be equal."""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, C, SIZE, BATCHES = 8, 5, 256, 80
HBM_PEAK = 8.0e12
BYTES_PER_PIXEL = 4 * C + 8                     # the logits row and the int64 label; no prediction map in validation


def from_stats(path):
    rows = []
    for f in glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        avg_ns = float(r.get("AverageNs") or 0.0)
        if "k_eval_overlap" in name and avg_ns > 0:
            b = BYTES_PER_PIXEL * N * SIZE * SIZE
            return {"avg_us": avg_ns / 1e3, "min_us": float(r.get("MinNs") or 0.0) / 1e3, "calls": int(float(r.get("Calls", 0))),
                    "algorithmic_MB": b / 1e6, "GB_per_s": b / avg_ns, "share_of_hbm_peak": b / (avg_ns * 1e-9) / HBM_PEAK}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--stats-csv", type=str, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.stats_csv:
        print(json.dumps({"k_eval_overlap": from_stats(args.stats_csv)}))
        return

    import types
    import torch
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    from smsut_amd.misc.synthetic import SyntheticSliceLoader
    from smsut_amd.misc.utils import Meter
    from smsut_amd.trainer.unetTrainer import UnetTrainer
    if not torch.cuda.is_available():
        raise SystemExit("profiles/validation_step.py measures on the GPU; none is visible")
    assert cfg.n_label + 1 == C and cfg.input_size == SIZE and cfg.batch_size == N
    torch.manual_seed(cfg.seed)
    tr = UnetTrainer("train", types.SimpleNamespace(fold=0, expr_name=None, write_env=False))
    loader = SyntheticSliceLoader(N, size=SIZE, n_batches=BATCHES, device=tr.device)
    state = loader.state_dict()

    def meter():
        return Meter([f"loss_{i}" for i in range(cfg.n_modal)] + ["loss"], [], alpha=1.0)

    def host():
        m = meter()
        gt = tr._collect_labels(loader)
        _, prd = tr.validate_epoch(loader, gt, m)
        return tr.validate_dice(prd, gt), m

    def device():
        m = meter()
        _, counter = tr.validate_epoch_device(loader, m)
        return tr.validate_dice_device(counter), m

    def forward():
        tr.net.eval()
        with torch.no_grad():
            for img, _, _, _ in loader:
                tr._forward_eval(img.to(tr.device))

    def loader_only():
        for _ in loader:
            pass

    def wall(fn):
        loader.load_state_dict(state)
        torch.cuda.synchronize()
        tic = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - tic, out

    if args.kernels_only:
        for _ in range(2):
            wall(device)
        return

    (_, (dice_h, meter_h)), (_, (dice_d, meter_d)) = wall(host), wall(device)         # warm-up round, and the equality check
    assert dice_h == dice_d and meter_h.cur_values == meter_d.cur_values and meter_h.n == meter_d.n, (dice_h, dice_d)
    legs = {"host": host, "device": device, "forward": forward, "loader": loader_only}
    wall(forward)
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                             # alternating
        for k, fn in legs.items():
            times[k].append(wall(fn)[0])
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    print(json.dumps({"device": torch.cuda.get_device_name(0), "shape": {"batches": BATCHES, "slices": N, "size": SIZE, "C": C},
                      "s_median": med, "s_all": times, "host_over_device": med["host"] / med["device"],
                      "device_minus_forward_s": med["device"] - med["forward"], "host_minus_forward_s": med["host"] - med["forward"],
                      "dice": dice_d["dice"], "equal_results": True}))


if __name__ == "__main__":
    main()
