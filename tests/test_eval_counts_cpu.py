"""``dice_matrix_from_counts`` against ``get_mo_matrix`` (misc/utils.py), no GPU: the counts {|P & G|, |P|, |G|} per (volume,
class) are formed here with NumPy from seeded random volumes, and the matrix from them must equal the matrix from the volumes
entry for entry (``==``: the same fp64 operations in the same order on equal integers, so no tolerance applies)."""
import numpy as np
import pytest

import smsut_amd  # noqa: F401
from smsut_amd import config as cfg
from smsut_amd.misc.utils import dice_matrix_from_counts, get_mo_matrix

SHAPE = (3, 16, 16)


def counts_of(prd, gt, keys, n_cls):
    """[len(keys), n_cls, 3] int64: what ops.eval_overlap accumulates (a truth label outside 0 .. n_cls-1 counts nowhere)."""
    out = np.zeros((len(keys), n_cls, 3), dtype=np.int64)
    for s, k in enumerate(keys):
        p, g = prd[k], gt[k]
        for c in range(n_cls):
            out[s, c] = (np.count_nonzero((p == c) & (g == c)), np.count_nonzero(p == c), np.count_nonzero(g == c))
    return out


def volumes(seed, keys, p_hi=5, g_hi=5, drop_p=(), drop_g=()):
    rs = np.random.RandomState(seed)
    prd, gt = {}, {}
    for k in keys:
        p = rs.randint(0, p_hi, SHAPE).astype(np.int64)
        g = rs.randint(0, g_hi, SHAPE).astype(np.int64)
        for c in drop_p:
            p[p == c] = 0
        for c in drop_g:
            g[g == c] = 0
        prd[k], gt[k] = p, g
    return prd, gt


CASES = {
    # every modality, one volume each
    "all-modalities": dict(keys=["ct_001", "t1in_002", "t1out_003", "t2_004"]),
    # class 3 in neither prediction nor truth: den == 0 -> 0.0
    "class-absent-from-both": dict(keys=["ct_001", "t2_004"], drop_p=(3,), drop_g=(3,)),
    # class 2 never predicted, present in the truth: 0 / |G|
    "class-absent-from-prediction": dict(keys=["ct_001", "t1in_002"], drop_p=(2,)),
    # t1in / t1out have no volume: the 1e-8 guard; ct has three volumes, t2 one, interleaved
    "empty-modalities-uneven-counts": dict(keys=["ct_001", "t2_004", "ct_005", "ct_009"]),
    # truth labels 5, 6 above n_label (and predictions stay in range)
    "truth-labels-above-n-label": dict(keys=["t1out_003", "ct_001", "t1out_008"], g_hi=7),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_matrix_from_counts_equals_get_mo_matrix(name):
    assert cfg.n_label == 4 and cfg.n_modal == 4
    case = dict(CASES[name])
    keys = case.pop("keys")
    prd, gt = volumes(sorted(CASES).index(name) + 11, keys, **case)
    if name == "class-absent-from-both":
        assert all((prd[k] != 3).all() and (gt[k] != 3).all() for k in keys)
    if name == "class-absent-from-prediction":
        assert all((prd[k] != 2).all() for k in keys) and any((gt[k] == 2).any() for k in keys)
    if name == "truth-labels-above-n-label":
        assert any((gt[k] > cfg.n_label).any() for k in keys)
    want = get_mo_matrix(prd, gt)
    got = dice_matrix_from_counts(keys, counts_of(prd, gt, keys, cfg.n_label + 1))
    assert got.shape == want.shape == (cfg.n_modal + 1, cfg.n_label + 1) and got.dtype == want.dtype
    assert (got == want).all(), (got, want)
    assert want[:cfg.n_modal, :cfg.n_label].max() > 0.0                  # (not a comparison of two zero matrices)
    # more classes counted than the matrix uses (CoraNet-style K > n_label + 1 never happens, but rows past n_label are ignored)
    assert (dice_matrix_from_counts(keys, counts_of(prd, gt, keys, 7)) == want).all()


def test_key_order_is_the_accumulation_order():
    """Per modality the volumes' scores are added in key order; fp64 addition is not associative, so the keys must be passed in
    the order ``get_mo_matrix`` walks its dict -- and then every entry is equal."""
    keys = [f"ct_{i:03d}" for i in range(7)] + ["t2_100"]
    prd, gt = volumes(5, keys)
    want = get_mo_matrix(prd, gt)
    assert (dice_matrix_from_counts(keys, counts_of(prd, gt, keys, 5)) == want).all()
    rev = keys[::-1]
    want_rev = get_mo_matrix({k: prd[k] for k in rev}, {k: gt[k] for k in rev})
    assert (dice_matrix_from_counts(rev, counts_of(prd, gt, rev, 5)) == want_rev).all()


def test_no_volume_at_all_and_fewer_classes_than_organs():
    want = get_mo_matrix({}, {})
    got = dice_matrix_from_counts([], np.zeros((0, 5, 3), dtype=np.int64))
    assert (got == want).all() and (got == 0.0).all()
    # a two-class network under n_label = 4: organs 2..4 are never predicted and score 0.0 in both
    keys = ["ct_001", "t1in_002"]
    prd, gt = volumes(3, keys, p_hi=2)
    assert (dice_matrix_from_counts(keys, counts_of(prd, gt, keys, 2)) == get_mo_matrix(prd, gt)).all()


def test_argument_checks():
    with pytest.raises(TypeError):
        dice_matrix_from_counts(["ct_001"], np.zeros((1, 5, 3)))                       # float counts
    with pytest.raises(ValueError):
        dice_matrix_from_counts(["ct_001"], np.zeros((2, 5, 3), dtype=np.int64))       # one key, two slots
    with pytest.raises(ValueError):
        dice_matrix_from_counts(["ct_001"], np.zeros((1, 5, 2), dtype=np.int64))
    with pytest.raises(KeyError):
        dice_matrix_from_counts(["mr_001"], np.zeros((1, 5, 3), dtype=np.int64))       # not a modality


def test_device_u8_refuses_tensors_that_are_not_device_uint8():
    """The matrix functions take device uint8 volumes as well as NumPy arrays; a CPU tensor or another dtype is refused on the
    host, before anything is uploaded."""
    import torch
    from smsut_amd.misc import utils
    for t in (torch.zeros(2, 4, 4, dtype=torch.uint8), torch.zeros(2, 4, 4), torch.zeros(2, 4, 4, dtype=torch.int64)):
        with pytest.raises(TypeError):
            utils._device_u8(t, "volume")
        with pytest.raises(TypeError):
            utils.get_all_matrix({"ct_001": t}, {"ct_001": t})
