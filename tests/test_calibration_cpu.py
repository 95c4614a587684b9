"""Host-side checks of the calibration feature: tests/calibration_ref.py against a plain torch composition, its fp32 emulation
inside its own budgets, the case draw, the Newton fit of the temperature in fp64, the metrics and the text of the csv.  No GPU."""
import numpy as np
import pytest
import torch

import calibration_ref as R


def composed(z, y, k, b, beta):
    """The totals from torch ops in fp64: softmax, max, bucketize-by-floor, bincount, cross_entropy, sums."""
    zt = torch.from_numpy(np.asarray(z, dtype=np.float32)).double().reshape(-1, z.shape[-1])[:, :k]
    yt = torch.from_numpy(np.asarray(y)).reshape(-1)
    keep = (yt >= 0) & (yt < k)
    zt, yk = zt[keep], yt[keep]
    p = torch.softmax(beta * zt, dim=1)
    conf, pred = p.max(dim=1)
    ok = (pred == yk).double()
    bins = torch.clamp((conf * b).floor().long(), max=b - 1)
    out = np.zeros(R.size(k, b))
    out[0:3 * b:3] = torch.bincount(bins, minlength=b).numpy()
    out[1:3 * b:3] = torch.bincount(bins, weights=conf, minlength=b).numpy()
    out[2:3 * b:3] = torch.bincount(bins, weights=ok, minlength=b).numpy()
    nll = torch.nn.functional.cross_entropy(beta * zt, yk, reduction="none")
    onehot = torch.nn.functional.one_hot(yk, k).double()
    brier = ((p - onehot) ** 2).sum(dim=1)
    for j, wgt in enumerate((torch.ones_like(ok), ok, nll, brier)):
        out[3 * b + j:3 * b + 4 * k:4] = torch.bincount(yk, weights=wgt, minlength=k).numpy()
    ez = (p * zt).sum(dim=1)
    out[3 * b + 4 * k] = (ez - zt.gather(1, yk[:, None])[:, 0]).sum()
    out[3 * b + 4 * k + 1] = ((p * zt * zt).sum(dim=1) - ez * ez).sum()
    out[3 * b + 4 * k + 2] = (~keep).sum()
    return out


@pytest.fixture(scope="module")
def drawn():
    return {case: R.draw(case, 500 + i) for i, case in enumerate(R.CASES + R.MORE_CASES)}


@pytest.mark.parametrize("case", R.CASES + R.MORE_CASES)
@pytest.mark.parametrize("temperature", (1.0, R.T_SCALED))
def test_reference_matches_a_plain_composition(drawn, case, temperature):
    z, y, _ = drawn[case]
    k, b = case[4:]
    beta = R.beta_of(temperature)
    want = composed(z, y, k, b, beta)
    got, _ = R.stats(z, y, k, b, beta)
    assert np.array_equal(got[0:3 * b:3], want[0:3 * b:3]) and np.array_equal(got[2:3 * b:3], want[2:3 * b:3])
    assert got[-1] == 0 and got[-2] == want[-2] and (got[-2] > 0) == (z[..., 0].size >= 6)
    assert np.allclose(got, want, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("case", R.CASES + R.MORE_CASES)
@pytest.mark.parametrize("temperature", (1.0, R.T_SCALED))
def test_emulation_stays_inside_the_budgets(drawn, case, temperature):
    z, y, _ = drawn[case]
    k, b = case[4:]
    beta = R.beta_of(temperature)
    ref, px = R.stats(z, y, k, b, beta)
    emu, _ = R.stats(z, y, k, b, beta, dtype=np.float32)
    tol = R.bounds(px, y, k, b, beta)
    exact = tol == 0
    assert np.array_equal(emu[exact], ref[exact])               # every count, every pixel: the draw left no borderline pixel
    err = np.abs(emu - ref)
    print(case, temperature, "largest err / bound", (err[~exact] / np.maximum(tol[~exact], 1e-300)).max())
    assert (err <= tol).all(), (err / np.maximum(tol, 1e-300)).max()


@pytest.mark.parametrize("case", R.CASES + R.MORE_CASES)
def test_draw_terminates_clear_of_every_bin_edge(drawn, case):
    z, y, rounds = drawn[case]
    n, h, w, c, k, b = case
    assert rounds <= 3
    betas = (1.0, R.beta_of(R.T_SCALED))
    assert not R.unsafe(z.reshape(-1, c), k, b, betas).any()
    for beta in betas:                                           # said once more without ``unsafe``: distance to the edges j / B
        _, px = R.stats(z, np.zeros_like(y), k, b, beta)
        conf = px["conf"]
        edges = np.arange(1, b) / b
        if edges.size:
            assert np.abs(conf[:, None] - edges[None, :]).min() > 4 * R.b_p(k, beta)
        assert px["gap"].min() >= 4 * R.b_p(k, beta)
    outside = (y < 0) | (y >= k)
    assert outside.sum() == len(range(5, n * h * w, 11))


def test_newton_fit_on_the_planted_case():
    import smsut_amd  # noqa: F401
    from smsut_amd.misc import utils
    z, y = R.planted(77)
    k = z.shape[-1]

    def evaluate(beta):
        _, g, h = R.newton_step_size(z, y, k, beta)
        return g, h

    beta, its = utils.newton_inverse_temperature(evaluate)
    t = 1.0 / beta
    print("planted 2.5x: fitted T", t, "after", its, "evaluations")
    assert its < 30 and 2.0 < t < 3.2
    step, _, _ = R.newton_step_size(z, y, k, R.beta_of(t))
    assert step <= 2e-6 * beta
    raw = utils.CalibrationTotals(R.stats(z, y, k, 15, 1.0)[0], k, 15)
    fit = utils.CalibrationTotals(R.stats(z, y, k, 15, R.beta_of(t))[0], k, 15)
    assert fit.nll() < raw.nll() and fit.ece() < raw.ece()


def test_newton_safeguard_halves():
    import smsut_amd  # noqa: F401
    from smsut_amd.misc import utils
    seen = []

    def evaluate(beta):                                          # a minimum at beta = 0.1 with a curvature that overshoots below 0
        seen.append(beta)
        return (beta - 0.1) * 1.0, (0.5 if len(seen) == 1 else 1.0)

    beta, its = utils.newton_inverse_temperature(evaluate)
    assert seen[1] == 0.5                                        # 1 - 0.9 / 0.5 < 0: halved
    assert abs(beta - 0.1) < 1e-6 and its < 30
    beta, its = utils.newton_inverse_temperature(lambda b: (0.0, 0.0), max_iter=3)    # h == 0: halved every time
    assert beta == 0.125 and its == 3


def test_metrics_of_a_totals_vector():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops
    from smsut_amd.misc import utils
    lay = ops.CalibrationLayout(2, 4)
    assert lay.size == 3 * 4 + 4 * 2 + 4
    v = np.zeros(lay.size)
    lay.bins(v)[:] = [[0, 0, 0], [0, 0, 0], [10, 6.0, 5], [30, 27.0, 30]]          # gaps |0.5 - 0.6|, |1 - 0.9|
    lay.classes(v)[:] = [[25, 20, 5.0, 2.5], [15, 15, 3.0, 1.5]]
    v[lay.size - 4:] = [1.5, 2.5, 3, 1]
    t = utils.CalibrationTotals(v, 2, 4)
    assert t.pixels == 40 and t.skipped() == 3 and t.nonfinite() == 1 and t.grad() == 1.5 and t.curv() == 2.5
    assert t.ece() == pytest.approx(0.25 * 0.1 + 0.75 * 0.1) and t.mce() == pytest.approx(0.1)
    assert t.nll() == pytest.approx(8.0 / 40) and t.brier() == pytest.approx(4.0 / 40) and t.accuracy() == pytest.approx(35 / 40)
    rel = t.reliability()
    assert rel.shape == (4, 5) and np.allclose(rel[:, 0], [0, .25, .5, .75]) and np.allclose(rel[:, 1], [.25, .5, .75, 1])
    assert np.isnan(rel[:2, 3:]).all() and np.allclose(rel[2:, 2:], [[10, 0.6, 0.5], [30, 0.9, 1.0]])
    assert np.allclose(t.per_class(), [[25, 0.8, 0.2, 0.1], [15, 1.0, 0.2, 0.1]])
    empty = utils.CalibrationTotals(np.zeros(lay.size), 2, 4)
    assert all(np.isnan(x) for x in empty.summary())
    with pytest.raises(ValueError):
        utils.CalibrationTotals(np.zeros(lay.size + 1), 2, 4)
    with pytest.raises(ValueError):
        ops.CalibrationLayout(33, 4)
    with pytest.raises(ValueError):
        ops.CalibrationLayout(2, 65)


def test_csv_text_layout():
    import smsut_amd  # noqa: F401
    from smsut_amd.misc import utils
    rel = np.array([[0.0, 0.5, 0, np.nan, np.nan], [0.5, 1.0, 12, 0.75, 0.5]])
    raw = np.array([[0.25, 0.25, 1.5, 0.5, 0.5], [np.nan] * 5, [0.25, 0.25, 1.5, 0.5, 0.5]])
    fit = raw * 0.5
    text = utils.calibration_text(rel, raw, fit)
    assert text == ("0.000000,0.500000,0.000000,nan,nan\n0.500000,1.000000,12.000000,0.750000,0.500000\n"
                    "\n"
                    "0.250000,0.250000,1.500000,0.500000,0.500000\nnan,nan,nan,nan,nan\n0.250000,0.250000,1.500000,0.500000,0.500000\n"
                    "\n"
                    "0.125000,0.125000,0.750000,0.250000,0.250000\nnan,nan,nan,nan,nan\n0.125000,0.125000,0.750000,0.250000,0.250000\n")
    blocks = text.split("\n\n")
    assert len(blocks) == 3 and len(utils.CALIBRATION_COLUMNS) == 5


def test_settings_default_off():
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    assert cfg.test_calibration is False and cfg.test_calibration_bins == 15


def test_read_temperature(tmp_path):
    import smsut_amd  # noqa: F401
    from smsut_amd import predict
    assert predict.read_temperature(None) is None and predict.read_temperature("1.75") == 1.75
    f = tmp_path / "temperature.txt"
    f.write_text(f"{2.4375!r}\n")
    assert predict.read_temperature(str(f)) == 2.4375
    assert predict.make_parser().parse_args(["--trainer", "unet", "-i", "0", "--image", "a", "--spacing", "1", "1", "1",
                                             "--modality", "ct", "--out", "o", "--temperature", "2"]).temperature == "2"
