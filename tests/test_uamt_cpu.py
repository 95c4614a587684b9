"""CPU checks of the uncertainty-aware mean teacher references (tests/uamt_ref.py) and of the fixture tests/golden/uamt.npz: the fp64
restatement against a literal transcription of the published composition, the derived entropy bound against an fp32 emulation of the
stated arithmetic, the threshold schedule, the case draw, and the fixture's arrays.  The device side (a fused loss head and a trainer)
is not in the tree yet; these are the references it will be held to."""
import math

import numpy as np
import torch

import uamt_ref as R


def published(outputs_ul, ema_output, preds, t, thr):
    """The published composition, line by line (train_uncertainty_aware_mean_teacher_2D.py of SSL4MIS): ``preds`` are the logits of
    the T stochastic passes written chunk after chunk into one [T * N, C, H, W] tensor."""
    n, c, h, w = outputs_ul.shape
    preds = torch.softmax(preds, dim=1)
    preds = preds.reshape(t, n, c, h, w)
    preds = torch.mean(preds, dim=0)
    uncertainty = -1.0 * torch.sum(preds * torch.log(preds + 1e-6), dim=1, keepdim=True)
    consistency_dist = (torch.softmax(outputs_ul, dim=1) - torch.softmax(ema_output, dim=1)) ** 2
    mask = (uncertainty < thr).float().to(outputs_ul.dtype)
    consistency_loss = torch.sum(mask * consistency_dist) / (2 * torch.sum(mask) + 1e-16)
    return consistency_loss, mask, uncertainty


def test_restatement_equals_the_published_composition():
    for shape in R.CASES[:6] + R.CASES[7:]:
        n, c, h, w, t = shape
        z, e, u = R.case(*shape)
        for thr in R.THRESHOLDS + (-1.0, float("inf")):
            zd = z.double().requires_grad_(True)
            out, mask, unc = R.loss_ref(zd, e, u, thr)
            out[0].backward()
            zp = z.double().requires_grad_(True)
            loss, pmask, punc = published(zp, e.double(), u.double().reshape(t * n, c, h, w), t, thr)
            loss.backward()
            assert abs(out[0].item() - loss.item()) <= 1e-14 * max(1.0, abs(loss.item())), (shape, thr)
            assert torch.equal(mask, pmask[:, 0] > 0) and (unc - punc[:, 0]).abs().max().item() <= 1e-14
            assert abs(out[1].item() - pmask.mean().item()) <= 1e-15 and abs(out[2].item() - punc.mean().item()) <= 1e-14
            assert (zd.grad - zp.grad).abs().max().item() <= 1e-15
            if thr == -1.0 and c > 1:
                assert out[0].item() == 0.0 and zd.grad.abs().max().item() == 0.0
            if thr == float("inf"):                            # every pixel kept: C / 2 times the mean teacher's term
                want = 0.5 * c * ((torch.softmax(z.double(), 1) - torch.softmax(e.double(), 1)) ** 2).mean().item()
                assert abs(out[0].item() - want) <= 1e-14


def test_mask_override_and_list_members():
    z, e, u = R.case(2, 5, 6, 7, 3)
    out, mask, h = R.loss_ref(z, e, list(u), R.THRESHOLDS[0])
    flipped = ~mask
    out2, m2, _ = R.loss_ref(z, e, u, R.THRESHOLDS[0], mask=flipped)
    assert torch.equal(m2, flipped) and abs(out2[1].item() + out[1].item() - 1.0) < 1e-15 and out2[2].item() == out[2].item()
    assert (h - R.entropy_ref(u)).abs().max().item() == 0.0


def test_case_draw_spreads_the_entropy():
    """the threshold actually cuts: at both thresholds a real share of the pixels is kept and a real share is dropped"""
    for shape in R.CASES[1:7]:
        n, c, h, w, t = shape
        _, _, u = R.case(*shape)
        hh = R.entropy_ref(u)
        assert hh.min().item() >= -1e-6 and hh.max().item() <= math.log(c) + 1e-12
        for thr in R.THRESHOLDS:
            kept = (hh < thr).double().mean().item()
            assert 0.05 <= kept <= 0.95, (shape, thr, kept)
    _, _, u = R.case(2, 1, 9, 7, 3)                            # one class: H = -log(1 + 1e-6) everywhere
    assert (R.entropy_ref(u) + math.log(1.0 + 1e-6)).abs().max().item() < 1e-15


def test_entropy_bound_values():
    assert abs(R.entropy_bound(5, 8) - 4.2e-6) < 1e-7 and abs(R.entropy_bound(10, 3) - 6.4e-6) < 1e-7
    assert 4.6e-8 < R.entropy_bound(1, 1) < 1e-6
    assert all(R.entropy_bound(c, t) < 1.1e-4 for c in range(1, 33) for t in range(1, 17))


def test_fp32_emulation_of_the_kernel_arithmetic_is_inside_the_bound():
    """B_H is derived, not fitted; this only shows that the stated arithmetic, emulated in numpy fp32, respects it"""
    for shape in R.CASES[:6] + R.CASES[7:]:
        n, c, h, w, t = shape
        _, _, u = R.case(*shape)
        err = float(np.abs(R.entropy_fp32(u).astype(np.float64) - R.entropy_ref(u).numpy()).max())
        print(shape, "fp32 emulation max |H - fp64| = %.2e, B_H = %.2e" % (err, R.entropy_bound(c, t)))
        assert err <= R.entropy_bound(c, t), (shape, err)


def test_threshold_schedule():
    max_it = 200 * 150
    assert abs(R.threshold(0, max_it) - (0.75 + 0.25 * math.exp(-5.0)) * math.log(2)) < 1e-15
    assert abs(R.threshold(max_it, max_it) - math.log(2)) < 1e-15 and abs(R.threshold(max_it - 1, max_it) - math.log(2)) < 1e-8
    assert R.threshold(0, max_it) - 0.75 * math.log(2) < 0.25 * math.exp(-5.0) + 1e-15       # 0.75 ln 2 up to the ramp-up's start value
    ts = [R.threshold(i, max_it) for i in range(0, max_it + 1, 1000)]
    assert all(a < b for a, b in zip(ts, ts[1:]))
    assert R.threshold(10, 100, 2.0) == 2.0 * R.threshold(10, 100, 1.0)
    import smsut_amd  # noqa: F401
    from smsut_amd.trainer.baseTrainer import BaseTrainer
    for i in (0, 7, 50, 100, 1000):
        assert R.rampup(i, 100) == BaseTrainer.sigmoid_rampup(i, 100)


def test_fixture_reproduces_from_uamt_ref(golden):
    g = golden("uamt")
    assert (int(g["C"]), int(g["width"]), int(g["H"]), int(g["bs"]), int(g["epoch"]), int(g["it0"])) == \
        (R.C, R.WIDTH, R.SIZE, R.BS, R.EPOCH, R.IT0)
    tm = float(g["threshold_max"])
    for k in range(2):
        assert abs(float(g["thr"][k]) - R.threshold(R.IT0 + k, R.MAX_IT, tm)) < 1e-15
    s32, s64 = g["scalars32"], g["scalars64"]
    assert s32.shape == s64.shape == (2, 4) and np.abs(s32 - s64).max() < 1e-4
    assert np.all((s64[:, 2] >= 0.3) & (s64[:, 2] <= 0.7)) and np.array_equal(s32[:, 2], s64[:, 2])     # kept; same mask in fp32 and fp64
    mask0 = np.unpackbits(g["mask0"])[:R.BS * R.SIZE * R.SIZE].reshape(R.BS, R.SIZE, R.SIZE).astype(bool)
    unc0 = g["unc0"].astype(np.float64)
    assert np.array_equal(mask0, unc0 < float(g["thr"][0])) and mask0.mean() == s64[0, 2]
    assert abs(unc0.mean() - s64[0, 3]) < 1e-6
    assert float(g["gap"]) > 0 and np.abs(unc0 - float(g["thr"][0])).min() >= float(g["gap"]) - 1e-6
    for k, name in R.POST.items():
        assert g["post32_" + k].shape == tuple(R.shapes()[name]) == g["post64_" + k].shape
    for i, shp in enumerate(R.HEAD_CASES):
        z, e, u = R.case(*shp)
        out, mask, _ = R.loss_ref(z, e, u, R.THRESHOLDS[0])
        assert np.abs(out.numpy() - g[f"head{i}_out"]).max() <= 1e-12, i
        assert np.array_equal(mask.numpy().astype(np.uint8), g[f"head{i}_mask"]), i
    img, msk, noise, mc = R.step_inputs(R.STEP_SEEDS[0])
    assert tuple(img.shape) == (2 * R.BS, 1, R.SIZE, R.SIZE) and tuple(mc.shape) == (R.MC_SAMPLES * R.BS, 1, R.SIZE, R.SIZE)
    clip = float(np.float32(R.NOISE_CLIP))
    assert noise.abs().max().item() <= clip and mc.abs().max().item() <= clip and 0.05 < mc.std().item() < 0.11
