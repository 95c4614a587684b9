"""Host-side checks of the test-time-augmentation feature (no GPU): the transform definition of tests/tta_ref.py, the named sets
of ``ops.tta_transforms``, the predictor's grouping plan and the command line of ``python -m smsut_amd.predict``."""
import itertools

import pytest
import torch

import tta_ref as R


def asym(h, w):
    """An array with no symmetry: every value differs."""
    return torch.arange(h * w, dtype=torch.float32).reshape(1, h, w) ** 1.5 + 3.0


def test_inverse_undoes_every_transform():
    x = asym(6, 6)
    for g in range(8):
        assert torch.equal(R.inv(R.fwd(x, g), g), x), g
    y = asym(5, 7)                                              # the flips on a non-square slice
    for g in (0, 4, 6, 2):
        assert R.fwd(y, g).shape == y.shape and torch.equal(R.inv(R.fwd(y, g), g), y), g


def test_the_eight_transforms_differ_pairwise():
    x = asym(6, 6)
    for a, b in itertools.combinations(range(8), 2):
        assert not torch.equal(R.fwd(x, a), R.fwd(x, b)), (a, b)


def test_flips_are_what_their_names_say():
    x = asym(5, 7)
    assert torch.equal(R.fwd(x, 4), torch.flip(x, [-1]))        # left-right
    assert torch.equal(R.fwd(x, 6), torch.flip(x, [-2]))        # up-down
    assert torch.equal(R.fwd(x, 2), torch.flip(x, [-2, -1]))    # both


def test_named_sets():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    assert ops.tta_transforms("none") == (0,)
    assert ops.tta_transforms("flips") == (0, 4, 6, 2)
    assert ops.tta_transforms("d4") == tuple(range(8))
    assert not any(g & 1 for g in ops.tta_transforms("flips"))  # no quarter turn: valid for any H x W
    assert ops.tta_transforms([5]) == (5,) and ops.tta_transforms((0, 0, 4, 4)) == (0, 0, 4, 4)
    for bad in ("rot", [], [8], [-1], list(range(8)) * 2 + [0]):
        with pytest.raises(ValueError):
            ops.tta_transforms(bad)
    for bad in (3, [1.0], [True], None):
        with pytest.raises(TypeError):
            ops.tta_transforms(bad)


def test_group_plan_covers_every_slice_once():
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    from smsut_amd.predict import Predictor, group_plan
    bs = cfg.batch_size
    p = Predictor(lambda x: x, tta="flips")
    assert p.batch_size == bs and p.members == 4
    for d in (1, bs - 1, bs, bs + 1, 3 * bs, 3 * bs + 2):
        plan = p.plan(d)
        assert plan == group_plan(d, bs)
        seen = [z for start, count, pad in plan for z in range(start, start + count)]
        assert seen == list(range(d)), d                        # every slice once, in order, the padding dropped
        assert all(count + pad == bs and count >= 1 for _, count, pad in plan)
        assert all(pad == 0 for _, _, pad in plan[:-1]) and plan[-1][2] == (-d) % bs
    with pytest.raises(ValueError):
        group_plan(0, bs)
    with pytest.raises(ValueError):                             # 3 networks x 8 transforms > 16 members
        Predictor([lambda x: x] * 3, tta="d4")


def test_cli_parser_accepts_the_documented_line():
    import smsut_amd  # noqa: F401
    from smsut_amd.predict import make_parser
    a = make_parser().parse_args("--trainer unet -i 000 -wh best --image scan.npy --spacing 5.0 1.5 1.25 --modality ct --tta flips "
                                 "--confidence --out out".split())
    assert (a.trainer, a.model_id, a.which_ckpt, a.image, a.modality, a.tta, a.confidence, a.out) == \
        ("unet", "000", "best", "scan.npy", "ct", "flips", True, "out")
    assert a.spacing == [5.0, 1.5, 1.25]
    b = make_parser().parse_args("--trainer crossPse -i 001 --image s.npy --spacing 1 1 1 --modality t2 --out o".split())
    assert (b.which_ckpt, b.tta, b.confidence) == ("last", "none", False)
    with pytest.raises(SystemExit):
        make_parser().parse_args("--trainer unet -i 000 --image s.npy --spacing 1 1 --modality ct --out o".split())
    with pytest.raises(SystemExit):
        make_parser().parse_args("--trainer unet -i 000 --image s.npy --spacing 1 1 1 --modality ct --tta rot --out o".split())


def test_merge_ref_on_a_case_done_by_hand():
    """Two members, identity and left-right flip, one row of two pixels, two classes."""
    z0 = torch.tensor([[[[0.0, 0.0], [2.0, 0.0]]]])             # [N=1, H=1, W=2, C=2]
    z1 = torch.tensor([[[[2.0, 0.0], [0.0, 0.0]]]])             # the flipped member: its pixel 0 is output pixel 1
    pred, conf, prob, gap = R.merge_ref([z0, z1], (0, 4))
    s = 1.0 / (1.0 + torch.exp(torch.tensor(-2.0, dtype=torch.float64)))
    assert torch.allclose(prob[0, 0, 0], torch.tensor([0.5, 0.5], dtype=torch.float64))
    assert torch.allclose(prob[0, 0, 1], torch.stack([s, 1 - s]))
    assert pred.tolist() == [[[0, 0]]]                          # a tie at pixel 0: the first maximum
    assert torch.allclose(conf[0, 0], torch.stack([torch.tensor(0.5, dtype=torch.float64), s]))
    assert gap[0, 0, 0] == 0 and torch.allclose(gap[0, 0, 1], 2 * s - 1)
    assert R.budget(5, 8) == 2.0 ** -24 * 26
