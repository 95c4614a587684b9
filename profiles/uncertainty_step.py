#!/usr/bin/env python3
"""Uncertainty maps and agreement counts: the fused pass (csrc/uncertainty.hip) against the same quantities composed from ATen ops,
and against the merge alone.

    python profiles/uncertainty_step.py            # timings, one JSON line (device events, alternating legs, after warm-up)

At 16 slices x 256 x 256 x 5 channels, T = 8 ('d4') and T = 4 ('flips'):
(1) ``ops.tta_uncertainty`` with the three maps and the counts;
(2) the ATen composition on the same device tensors: softmax per member, inverse flip / rot90, stack, mean, the entropies, the
    argmax of every member, comparisons and sums for the votes and the counts -- what a script built from torch would launch;
(3) ``ops.tta_merge`` alone (prediction + confidence): what the uncertainty adds to the existing pass.
The comparison is always against (2) and (3), never against the fused path itself.  Algorithmic bytes come from the shapes:
T * C * 4 in, 1 + 4 + 4 + 4 + 1 out per pixel (the counts are a few hundred bytes)."""
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
    return N * SIZE * SIZE * (t * C * 4 + 1 + 4 + 4 + 4 + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import torch
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("profiles/uncertainty_step.py measures on the GPU; none is visible")
    import tta_ref as R
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    sets = {8: ops.tta_transforms("d4"), 4: ops.tta_transforms("flips")}
    # a shared per-pixel logit vector of random sharpness plus unit member noise (as the tests draw): the members partly agree
    shared = 3 * torch.randn(N, SIZE, SIZE, C, generator=g) * (1.5 * torch.rand(N, SIZE, SIZE, 1, generator=g))
    members = [R.fwd((shared + torch.randn(N, SIZE, SIZE, C, generator=g)).permute(0, 3, 1, 2), gg).permute(0, 2, 3, 1)
               .contiguous().to(dev).permute(0, 3, 1, 2) for gg in sets[8]]
    members4 = [R.fwd(R.inv(m, g8), g4).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
                for m, g8, g4 in zip(members, sets[8], sets[4])]
    mem = {8: members, 4: members4}
    counts = {t: torch.zeros(C, 2 * t + 4, dtype=torch.int64, device=dev) for t in sets}
    scale = float(ops.UNCERTAIN_ENTROPY_SCALE)

    def fused(t):
        def run():
            counts[t].zero_()
            return ops.tta_uncertainty(mem[t], sets[t], counts=counts[t]), counts[t]
        return run

    def aten(t):
        def run():
            ps = torch.stack([R.inv(torch.softmax(z, dim=1), gg) for z, gg in zip(mem[t], sets[t])])      # [T, N, C, H, W]
            lab = torch.stack([R.inv(z.argmax(dim=1), gg) for z, gg in zip(mem[t], sets[t])])            # [T, N, H, W]
            mean = ps.mean(0)
            conf, pred = mean.max(dim=1)
            h = -(mean * torch.log(mean + 1e-6)).sum(1)
            eh = -(ps * torch.log(ps + 1e-6)).sum(2).mean(0)
            mi = (h - eh).clamp_min(0)
            agree = lab == pred
            votes = agree.sum(0).to(torch.uint8)
            onehot_p = torch.nn.functional.one_hot(pred, C)                                              # [N, H, W, C]
            onehot_l = torch.nn.functional.one_hot(lab, C)                                               # [T, N, H, W, C]
            out = torch.empty(C, 2 * t + 4, dtype=torch.int64, device=dev)
            out[:, 0] = onehot_p.sum((0, 1, 2))
            out[:, 1] = onehot_l.all(0).sum((0, 1, 2))
            out[:, 2] = onehot_l.any(0).sum((0, 1, 2))
            out[:, 3] = (onehot_p * torch.round(h * scale).long().unsqueeze(-1)).sum((0, 1, 2))
            out[:, 4:4 + t] = onehot_l.sum((1, 2, 3)).t()
            out[:, 4 + t:] = (onehot_l * agree.unsqueeze(-1)).sum((1, 2, 3)).t()
            return (pred.to(torch.uint8), conf, h, mi, votes), out
        return run

    def merge(t):
        return lambda: ops.tta_merge(mem[t], sets[t], want_conf=True)

    check = {}
    for t in (8, 4):                                           # same quantities, before any timing
        (u, cu), (a, ca) = fused(t)(), aten(t)()
        same_pred = u.pred == a[0]
        check[t] = {"pred_mismatch": int((~same_pred).sum()),
                    "max_entropy_diff": float((u.entropy - a[2]).abs().max()), "max_mi_diff": float((u.mutual_info - a[3]).abs().max()),
                    "votes_mismatch_where_pred_agrees": int(((u.votes != a[4]) & same_pred).sum()),
                    "member_voxels_equal": bool(torch.equal(cu[:, 4:4 + t], ca[:, 4:4 + t])),
                    "any_all_equal": bool(torch.equal(cu[:, 1:3], ca[:, 1:3])),
                    "max_count_diff": int((cu - ca)[:, [0] + list(range(4 + t, 4 + 2 * t))].abs().max())}
        assert check[t]["max_entropy_diff"] < 1e-5 and check[t]["max_mi_diff"] < 1e-5 and check[t]["pred_mismatch"] <= 16, check
        assert check[t]["votes_mismatch_where_pred_agrees"] == 0 and check[t]["member_voxels_equal"] and check[t]["any_all_equal"], check
        assert check[t]["max_count_diff"] <= 16, check

    def timed(fn, iters):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        for _ in range(iters):
            fn()
        en.record()
        torch.cuda.synchronize()
        return st.elapsed_time(en) / iters * 1e3               # us per call

    legs = {}
    for t in (8, 4):
        legs[f"uncertain{t}_fused"], legs[f"uncertain{t}_aten"], legs[f"merge{t}"] = fused(t), aten(t), merge(t)
        # where the fused pass spends what it adds: the maps without the counts, the counts without the maps
        legs[f"uncertain{t}_maps_only"] = (lambda t: lambda: ops.tta_uncertainty(mem[t], sets[t]))(t)
        legs[f"uncertain{t}_counts_only"] = (lambda t: lambda: ops.tta_uncertainty(mem[t], sets[t], counts=counts[t], want_maps=False))(t)
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):                               # alternating
        for k, fn in legs.items():
            times[k].append(timed(fn, args.iters))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    out = {"device": torch.cuda.get_device_name(0), "shape": {"slices": N, "size": SIZE, "C": C}, "us_median": med, "us_all": times,
           "check_vs_aten": check, "note": "the fused leg includes zeroing its counts (one small launch)"}
    for t in (8, 4):
        b = algorithmic_bytes(t)
        rate = b / (med[f"uncertain{t}_fused"] * 1e-6)
        out[f"uncertain{t}"] = {"algorithmic_MB": b / 1e6, "bytes_per_pixel": b / (N * SIZE * SIZE), "GB_per_s": rate / 1e9,
                                "share_of_hbm_peak": rate / HBM_PEAK, "us_at_hbm_peak": b / HBM_PEAK * 1e6,
                                "speedup_vs_aten": med[f"uncertain{t}_aten"] / med[f"uncertain{t}_fused"],
                                "times_the_merge_alone": med[f"uncertain{t}_fused"] / med[f"merge{t}"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
