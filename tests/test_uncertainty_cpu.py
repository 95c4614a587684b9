"""Host side of the uncertainty maps and quality scores: the references of tests/uncertainty_ref.py against their own bounds,
``misc.utils.structure_agreement``, the counts layout, the argument checks of ``ops.tta_uncertainty`` that fire before any device
use, and the command line.  No GPU."""
import math

import numpy as np
import pytest
import torch

import tta_ref
import uamt_ref
import uncertainty_ref as U


# ---------------------------------------------------------------------------------------------- the emulation and its bounds
@pytest.mark.parametrize("n,c,h,w,t", uamt_ref.CASES + [(1, 32, 12, 12, 16)],
                         ids=[f"N{n}-C{c}-{h}x{w}-T{t}" for n, c, h, w, t in uamt_ref.CASES + [(1, 32, 12, 12, 16)]])
def test_emulation_within_bounds(n, c, h, w, t):
    """numpy's exp / log are not the device's, but the bounds allow 2 ulp for each: an emulation outside them means a bound, or the
    stated arithmetic, is wrong."""
    _, _, mem = uamt_ref.case(n, c, h, w, t)                                    # [T, N, C, H, W], identity transforms
    members = [m.permute(0, 2, 3, 1).contiguous().numpy() for m in mem]
    tr = (0,) * t
    _, _, h64, eh64, mi64, _ = U.reference(members, tr, c)
    _, _, h32, eh32, mi32 = U.emulate_fp32(members, tr, c)
    assert np.array_equal(h32, uamt_ref.entropy_fp32(mem))                      # the same arithmetic as the UA-MT reference states
    err = lambda a, b: float(np.abs(a.astype(np.float64) - b.numpy()).max())
    eh, eeh, emi = err(h32, h64), err(eh32, eh64), err(mi32, mi64)
    print(f"emulation C={c} T={t}: |H| {eh:.2e} <= {U.bound_h(c, t):.2e}, |EH| {eeh:.2e} <= {U.bound_eh(c, t):.2e}, "
          f"|MI| {emi:.2e} <= {U.bound_mi(c, t):.2e}; H in [{float(h64.min()):.3f}, {float(h64.max()):.3f}], ln C = {math.log(c):.3f}")
    assert eh <= U.bound_h(c, t) and eeh <= U.bound_eh(c, t) and emi <= U.bound_mi(c, t)
    assert float(mi64.min()) >= -1e-12                                          # the true mutual information is not negative
    if t == 1:
        assert np.all(mi32 == 0)


@pytest.mark.parametrize("idx", range(len(U.CASES)), ids=U.IDS)
def test_gpu_cases_are_decided_by_the_reference(idx):
    """The seed of the GPU cases: the fp64 reference alone leaves at most 0.5 % of a case's pixels with a top-two gap below
    4 x budget, and the transformed draw, put back, is the emulation's input (F_g^-1 F_g = identity)."""
    t, n, h, w, c, k, tr, off = U.CASES[idx]
    members = U.draw_cases()[idx]
    assert len(members) == t and all(m.shape == ((n, w, h, c) if g & 1 else (n, h, w, c)) for m, g in zip(members, tr))
    pred, conf, h64, eh64, mi64, gap = U.reference(members, tr, k)
    assert float((gap < 4 * tta_ref.budget(k, t)).double().mean()) <= 0.005
    p32, _, h32, _, mi32 = U.emulate_fp32(members, tr, k)
    assert float(np.abs(h32 - h64.numpy()).max()) <= U.bound_h(k, t)
    assert float(np.abs(mi32 - mi64.numpy()).max()) <= U.bound_mi(k, t)
    decided = (gap >= 4 * tta_ref.budget(k, t)).numpy()
    assert np.array_equal(p32[decided], pred.numpy()[decided])
    if k > 1 and n * h * w >= 100:                                              # the draw spreads H over most of [0, ln K]
        assert float(h64.min()) < 0.25 * math.log(k) and float(h64.max()) > 0.75 * math.log(k)


# ---------------------------------------------------------------------------------------------- counts: layout and reference
def test_counts_layout_and_reference():
    from smsut_amd import ops
    lay = ops.UncertaintyLayout(3)
    assert (lay.V, lay.ALL, lay.ANY, lay.HSUM, lay.slots) == (U.V, U.ALL, U.ANY, U.HSUM, 2 * 3 + 4) and U.FIXED == 4
    assert ops.UNCERTAIN_ENTROPY_SCALE == U.SCALE == 2 ** 20
    # 1 x 1 x 4 pixels, two classes, three members
    pred = np.array([[[0, 1, 1, 0]]])
    labels = np.array([[[[0, 1, 1, 1]]], [[[0, 1, 0, 0]]], [[[0, 0, 1, 0]]]])
    h = np.array([[[0.25, 0.5, np.nan, 2.0 ** -20]]], dtype=np.float32)
    c = U.counts_of(pred, labels, h, 2)
    assert c.shape == (2, 10) and c.dtype == np.int64
    assert c[0].tolist() == [2, 1, 4, 2 ** 18 + 1, 1, 3, 3, 1, 2, 2]          # V ALL ANY HSUM V_0..2 I_0..2
    assert c[1].tolist() == [2, 0, 3, 2 ** 19, 3, 1, 1, 2, 1, 1]              # (the NaN pixel counts everywhere but in HSUM)
    assert np.array_equal(lay.member_voxels(c), c[:, 4:7]) and np.array_equal(lay.member_overlap(c), c[:, 7:10])
    assert U.votes_of(labels, pred).tolist() == [[[3, 2, 2, 2]]]
    assert U.first_max(np.array([[1.0, 3.0, 3.0], [np.nan, 5.0, np.nan], [2.0, np.nan, 9.0]])).tolist() == [1, 0, 1]
    with pytest.raises(ValueError):
        ops.UncertaintyLayout(17)
    with pytest.raises(TypeError):
        ops.UncertaintyLayout(2.0)


# ---------------------------------------------------------------------------------------------- structure_agreement
def test_structure_agreement_by_hand():
    from smsut_amd.misc.utils import QUALITY_COLUMNS, format_quality_csv, structure_agreement
    #        V  ALL ANY HSUM        V_0 V_1  I_0 I_1
    c = np.array([[10, 6, 14, 5 * 2 ** 20, 8, 12, 7, 9],
                  [4, 4, 4, 0, 4, 4, 4, 4],
                  [0, 0, 3, 0, 3, 0, 0, 0],                                    # never predicted, one member saw it
                  [0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int64)                   # absent altogether
    q = structure_agreement(c, 2)
    assert np.allclose(q.dice_agreement[:2], [(2 * 7 / 18 + 2 * 9 / 22) / 2, 1.0], rtol=0, atol=1e-15)
    assert np.isnan(q.dice_agreement[3]) and np.isnan(q.dice_agreement[2])     # member 1: 0 / (0 + 0)
    assert np.allclose(q.iou_all[:3], [6 / 14, 1.0, 0.0], rtol=0, atol=1e-15) and np.isnan(q.iou_all[3])
    assert np.allclose(q.volume_cv[:3], [2.0 / 10.0, 0.0, 1.0], rtol=0, atol=1e-15) and np.isnan(q.volume_cv[3])
    assert q.mean_entropy[0] == 0.5 and q.mean_entropy[1] == 0.0 and np.isnan(q.mean_entropy[2]) and np.isnan(q.mean_entropy[3])
    assert q.voxels.dtype == np.int64 and q.voxels.tolist() == [10, 4, 0, 0]
    assert all(a.dtype == np.float64 for a in q[:4])
    same = structure_agreement(torch.from_numpy(c), 2)                          # a tensor is as good
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(q, same))
    text = format_quality_csv(q).splitlines()
    assert text[0] == ",".join(QUALITY_COLUMNS) and len(text) == 5
    assert text[2] == "1,4,1.000000,1.000000,0.000000,0.000000" and text[4] == "3,0,nan,nan,nan,nan"
    assert format_quality_csv(q, names=list("abcd")).splitlines()[1].startswith("a,10,")
    with pytest.raises(ValueError):
        structure_agreement(c, 3)                                              # 8 columns are not 2 * 3 + 4
    with pytest.raises(TypeError):
        structure_agreement(c.astype(np.float64), 2)
    with pytest.raises(ValueError):
        format_quality_csv(q, names=["a"])


# ---------------------------------------------------------------------------------------------- refusals before any device use
def test_tta_uncertainty_refuses_on_the_host():
    from smsut_amd import ops
    z = torch.zeros(1, 5, 4, 4)
    with pytest.raises(TypeError):                              # a CPU tensor: no fallback
        ops.tta_uncertainty([z], (0,))
    with pytest.raises(TypeError):                              # fp16 logits
        ops.tta_uncertainty([z.half()], (0,))
    with pytest.raises(TypeError):                              # not tensors
        ops.tta_uncertainty([None], (0,))
    with pytest.raises(TypeError):
        ops.tta_uncertainty(5, (0,))
    with pytest.raises(ValueError):                             # T = 17
        ops.tta_uncertainty([z] * 17, [0] * 16)
    with pytest.raises(ValueError):                             # a transform outside 0..7
        ops.tta_uncertainty([z], (8,))
    with pytest.raises(ValueError):
        ops.tta_uncertainty([z], "d8")
    with pytest.raises(TypeError):                              # counts of the wrong type, found before the members are looked at
        ops.tta_uncertainty([z], (0,), counts=np.zeros((5, 6), dtype=np.int64))
    with pytest.raises(TypeError):
        ops.tta_uncertainty([z], (0,), counts=torch.zeros(5, 6, dtype=torch.int32))


def test_cli_flag_parses():
    from smsut_amd import predict
    base = "--trainer unet -i 000 --image scan.npy --spacing 5.0 1.5 1.5 --modality ct --out out".split()
    assert predict.make_parser().parse_args(base).uncertainty is False
    args = predict.make_parser().parse_args(base + ["--uncertainty", "--tta", "d4"])
    assert args.uncertainty is True and args.tta == "d4" and args.confidence is False
    assert predict.PredictResult._fields == ("labels", "labels_processed", "confidence", "plan")
    assert predict.UncertainResult._fields[:4] == predict.PredictResult._fields
    assert {"entropy", "mutual_info", "votes", "quality"} <= set(predict.UncertainResult._fields)
    assert predict.UncertainSlices._fields == ("pred", "conf", "entropy", "mutual_info", "votes", "counts")
