"""Host-side checks of sliding-window inference (no GPU): ``ops.window_plan`` and ``ops.window_weights``, the fp64 restatement of
tests/window_ref.py, every error ``ops.window_blend``, ``Predictor.predict_windows``, ``prepare_volume(field_of_view=...)`` and
``predict_volume`` raise before the device is touched, and the command line's new options."""
import math

import numpy as np
import pytest
import torch

import window_ref as R


@pytest.fixture(scope="module")
def ops():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    return ops


def test_window_plan_worked_examples(ops):
    assert ops.window_plan(52, 24, 0.5) == (0, 9, 18, 28)
    assert ops.window_plan(40, 24, 0.5) == (0, 8, 16)
    assert len(ops.window_plan(20, 8, 0.75)) == 7
    assert ops.window_plan(24, 24, 0.5) == (0,) and ops.window_plan(256, 256) == (0,)
    assert ops.window_plan(334, 256) == (0, 78) and ops.window_plan(512, 256) == (0, 128, 256)


def test_window_plan_properties(ops):
    seen = 0
    for window in (1, 2, 3, 7, 8, 12, 24, 32):
        for size in list(range(window, window + 40)) + [5 * window + 3, 16 * window]:
            for overlap in (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99):
                pos = ops.window_plan(size, window, overlap)
                target = max(1, int(window * (1 - overlap)))
                assert pos[0] == 0 and pos[-1] == size - window, (size, window, overlap, pos)
                assert all(isinstance(p, int) for p in pos)
                steps = [b - a for a, b in zip(pos, pos[1:])]
                assert all(1 <= s <= target for s in steps), (size, window, overlap, pos)      # strictly increasing, every index covered
                assert len(pos) == math.ceil((size - window) / target) + 1
                assert pos == R.plan(size, window, overlap)
                seen += 1
    assert seen > 2000


def test_window_plan_refuses(ops):
    for size, window, overlap in ((8, 9, 0.5), (8, 0, 0.5), (0, 0, 0.5), (8, 4, 1.0), (8, 4, -0.1), (8, 4, float("nan"))):
        with pytest.raises(ValueError):
            ops.window_plan(size, window, overlap)
    for size, window, overlap in ((8.0, 4, 0.5), (8, True, 0.5), (8, 4, "half"), (8, 4, None)):
        with pytest.raises(TypeError):
            ops.window_plan(size, window, overlap)


def test_window_weights(ops):
    for n in (1, 2, 7, 8, 24, 255, 256):
        w = ops.window_weights(n, "gaussian")
        assert w.dtype == torch.float32 and tuple(w.shape) == (n,) and w.device.type == "cpu"
        formula = [math.exp(-0.5 * ((i - (n - 1) / 2) / (n / 8)) ** 2) for i in range(n)]
        assert torch.equal(w, torch.tensor(formula, dtype=torch.float64).float()), n             # fp64, rounded once
        assert torch.equal(w, torch.flip(w, [0])) and bool(torch.isfinite(w).all()) and float(w.min()) > 0
        assert np.array_equal(w.numpy(), R.weights(n, "gaussian"))
        assert torch.equal(ops.window_weights(n, "constant"), torch.ones(n))
    w = ops.window_weights(256, "gaussian")
    assert abs(float(w.min()) - 3.6e-4) < 1e-5 and float(w.max()) == float(np.float32(math.exp(-0.5 * (0.5 / 32) ** 2)))
    corner = float(w[0] * w[0])
    assert abs(corner - 1.3e-7) < 1e-8 and corner > float(np.finfo(np.float32).tiny)             # a normal fp32 number
    with pytest.raises(ValueError):
        ops.window_weights(8, "triangle")
    with pytest.raises(ValueError):
        ops.window_weights(0, "gaussian")
    with pytest.raises(TypeError):
        ops.window_weights(8.0, "gaussian")


def test_blend_ref_identities():
    rng = np.random.default_rng(5)
    one = torch.softmax(torch.from_numpy(rng.standard_normal((2, 6, 7, 5))), dim=-1).float()
    pred, conf, prob, gap, cover = R.blend_ref([one], (0,), (0,), (6, 7), R.weights(6, "gaussian"), R.weights(7, "gaussian"))
    assert cover == 1 and torch.equal(prob, one.double())                                        # one tile is the identity
    assert torch.equal(pred, R.first_max(one.double())) and torch.equal(conf, one.double().max(dim=-1).values)
    assert R.budget(1) == 2.0 ** -24 * 4 and R.budget(16) == 2.0 ** -24 * 34
    # identical tiles: whatever the weights, the blend returns the tile
    ys, xs = R.plan(14, 8, 0.5), R.plan(17, 8, 0.5)
    full = torch.softmax(torch.from_numpy(rng.standard_normal((1, 14, 17, 4))), dim=-1).float()
    tiles = [full[:, y0:y0 + 8, x0:x0 + 8] for y0 in ys for x0 in xs]
    for blend in ("gaussian", "constant"):
        wt = R.weights(8, blend)
        _, _, prob, _, cover = R.blend_ref(tiles, ys, xs, (14, 17), wt, wt)
        assert cover == 9 and float((prob - full.double()).abs().max()) <= R.budget(cover), blend
    # two tiles, constant weights: the overlap is the plain mean, by hand
    a, b = torch.full((1, 1, 3, 2), 0.25), torch.full((1, 1, 3, 2), 0.75)
    _, _, prob, gap, cover = R.blend_ref([a, b], (0,), (0, 1), (1, 4), np.ones(1, np.float32), np.ones(3, np.float32))
    assert cover == 2 and prob[0, 0, :, 0].tolist() == [0.25, 0.5, 0.5, 0.75] and float(gap.max()) == 0


@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=R.IDS)
def test_reference_decides_every_pixel(idx):
    """The cases of tests/test_window_gpu.py: with the committed seed no pixel's two largest probabilities are within 4 budgets."""
    c = R.cases()[idx]
    expect_cover = {0: 9, 2: 16}
    assert len(c.tiles) == len(c.ys) * len(c.xs) and (idx not in expect_cover or c.cover == expect_cover[idx])
    if idx == 2:
        assert len(c.tiles) == 49
    print(f"{R.IDS[idx]}: {len(c.ys)} x {len(c.xs)} tiles, cover {c.cover}, smallest gap {float(c.gap.min()):.3e}, 4 B = {4 * c.budget:.3e}")
    assert float(c.gap.min()) >= 4 * c.budget


def tiles_for(n, h, w, win, k, overlap=0.5):
    ys, xs = R.plan(h, win, overlap), R.plan(w, win, overlap)
    return [torch.zeros(n, win, win, k) for _ in range(len(ys) * len(xs))], ys, xs


def test_window_blend_refuses_on_the_host(ops):
    wt = torch.ones(8)
    tiles, ys, xs = tiles_for(1, 12, 14, 8, 3)
    ok = (tiles, ys, xs, (12, 14), wt, wt)
    for bad in ((tiles[:-1] + [np.zeros((1, 8, 8, 3), np.float32)],) + ok[1:],                   # not a tensor
                (tiles[:-1] + [tiles[-1].double()],) + ok[1:],                                   # not fp32
                (tiles[:-1] + [tiles[-1].half()],) + ok[1:],
                ok[:4] + (wt.double(), wt), ok[:4] + (wt, [1.0] * 8), (3,) + ok[1:],
                (tiles, (0, 4.0)) + ok[2:], (tiles, ys, None) + ok[3:],
                ok):                                                                             # all well, but on the CPU
        with pytest.raises(TypeError):
            ops.window_blend(*bad)
    sliced = torch.zeros(1, 8, 8, 6)[..., :3]                                                    # right shape, not contiguous
    for bad in ((tiles[:-1] + [sliced],) + ok[1:],
                (tiles[:-1] + [torch.zeros(1, 8, 7, 3)],) + ok[1:],
                ([t[0] for t in tiles],) + ok[1:],                                               # [wh, ww, K]
                (tiles[:-1],) + ok[1:], (tiles + tiles[:1],) + ok[1:], ([],) + ok[1:],           # a count that is not ny * nx
                (tiles, (0, 0)) + ok[2:], (tiles, (4, 0)) + ok[2:],                              # not strictly increasing
                (tiles, (0, 5)) + ok[2:], (tiles, (-1, 4)) + ok[2:],                             # outside the grid
                (tiles, (1, 4)) + ok[2:], (tiles, (0, 3)) + ok[2:],                              # index 0 / index 11 uncovered
                (tiles, ys, xs, (12, 7), wt, wt), (tiles, ys, xs, (12,), wt, wt),
                ok[:4] + (torch.ones(7), wt), ok[:4] + (wt, torch.ones(8, 1)),                   # tables of the wrong length
                ([torch.zeros(1, 8, 8, 33)] * 4,) + ok[1:]):                                     # 33 classes
        with pytest.raises(ValueError):
            ops.window_blend(*bad)
    many, mys, mxs = tiles_for(1, 8 + 12 * 2, 8 + 4 * 2, 8, 2, overlap=0.75)                     # 13 x 5 = 65 tiles
    assert len(many) == 65
    with pytest.raises(ValueError, match="at most 64"):
        ops.window_blend(many, mys, mxs, (32, 16), wt, wt)
    gap_tiles = [torch.zeros(1, 8, 8, 3)] * 2                                                    # rows 8..9 under no tile
    with pytest.raises(ValueError, match="uncovered"):
        ops.window_blend(gap_tiles, (0, 10), (0,), (18, 8), wt, wt)


def test_predict_windows_refuses_on_the_host():
    import smsut_amd  # noqa: F401
    from smsut_amd.predict import Predictor
    p = Predictor(lambda x: x, batch_size=2, tta="d4")
    img = torch.zeros(3, 20, 24, dtype=torch.uint8)
    for bad in ((img.float(), 8), (img.numpy(), 8), (img, 8.0), (img, True), (img, 8, "half")):
        with pytest.raises(TypeError):
            p.predict_windows(*bad)
    for bad in ((img[0], 8), (img, 21), (img, 0), (img, 8, 1.0), (img, 8, -0.5), (img, 8, 0.5, "triangle"),
                (img, 2, 0.5)):                                                                  # 19 x 23 windows: more than 64
        with pytest.raises(ValueError):
            p.predict_windows(*bad)
    with pytest.raises(TypeError, match="HIP device"):                                           # all well, but on the CPU
        p.predict_windows(img, 8)


def test_field_of_view_is_checked_before_anything_else():
    import smsut_amd  # noqa: F401
    from smsut_amd.data_pprocess.volume import FIELDS_OF_VIEW, prepare_volume
    from smsut_amd.predict import Predictor, predict_volume
    assert FIELDS_OF_VIEW == ("crop", "full")
    vol = np.zeros((2, 8, 8), np.float32)
    with pytest.raises(ValueError, match="field_of_view"):
        prepare_volume(vol, None, (5.0, 1.5, 1.5), "ct", field_of_view="whole")
    p = Predictor(lambda x: x)
    with pytest.raises(ValueError, match="field_of_view"):
        predict_volume(p, vol, (5.0, 1.5, 1.5), "ct", field_of_view="whole")
    with pytest.raises(ValueError, match="uncertainty"):
        predict_volume(p, vol, (5.0, 1.5, 1.5), "ct", uncertainty=True, field_of_view="full")


def test_cli_parser_takes_the_field_of_view():
    import smsut_amd  # noqa: F401
    from smsut_amd.predict import make_parser
    base = "--trainer unet -i 000 --image scan.npy --spacing 0.8 0.98 0.98 --modality ct --out out"
    a = make_parser().parse_args(base.split())
    assert (a.field_of_view, a.overlap, a.blend) == ("crop", 0.5, "gaussian")                    # the defaults: today's path
    b = make_parser().parse_args((base + " --field-of-view full --overlap 0.25 --blend constant").split())
    assert (b.field_of_view, b.overlap, b.blend) == ("full", 0.25, "constant")
    for bad in ("--field-of-view whole", "--blend triangle", "--overlap wide"):
        with pytest.raises(SystemExit):
            make_parser().parse_args((base + " " + bad).split())
