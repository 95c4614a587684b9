"""``ops.calibration_stats`` (csrc/calibration.hip) against the fp64 reference of tests/calibration_ref.py: every count exact, every
float total inside its derived bound, planted exact cases, bitwise reproducibility, the temperature fit, and the refusals."""
import numpy as np
import pytest
import torch

import calibration_ref as R

pytestmark = pytest.mark.gpu

TEMPS = (1.0, R.T_SCALED)


def nchw(z, offset=0):
    """NumPy [N, H, W, C] -> the logical NCHW device tensor in NHWC memory; ``offset``: floats into its allocation it starts at."""
    flat = torch.empty(z.size + offset, dtype=torch.float32, device="cuda")
    flat[offset:] = torch.from_numpy(z).reshape(-1)
    return flat[offset:].view(*z.shape).permute(0, 3, 1, 2)


def run(z, y, k, b, temperature, out=None, offset=0):
    from smsut_amd import ops
    if out is None:
        out = torch.zeros(ops.CalibrationLayout(k, b).size, dtype=torch.float64, device="cuda")
    copies = ops.layout_copies()
    ops.calibration_stats(nchw(z, offset), torch.from_numpy(y).cuda(), out, classes=k, bins=b, temperature=temperature)
    assert ops.layout_copies() == copies
    return out


ALL_CASES = R.CASES + R.MORE_CASES


@pytest.fixture(scope="module")
def drawn():
    return {case: R.draw(case, 500 + i) for i, case in enumerate(ALL_CASES)}


def check(got, z, y, k, b, temperature, what):
    beta = R.beta_of(temperature)
    ref, px = R.stats(z, y, k, b, beta)
    tol = R.bounds(px, y, k, b, beta)
    exact = tol == 0
    err = np.abs(got - ref)
    print(what, "T", temperature, "largest err / bound", (err[~exact] / np.maximum(tol[~exact], 1e-300)).max(initial=0.0))
    assert np.array_equal(got[exact], ref[exact]), (what, got[exact], ref[exact])
    assert (err <= tol).all(), (what, (err / np.maximum(tol, 1e-300)).max())
    return ref


@pytest.mark.parametrize("case", ALL_CASES)
def test_against_fp64(drawn, case):
    from smsut_amd import ops
    z, y, _ = drawn[case]
    n, h, w, c, k, b = case
    lay = ops.CalibrationLayout(k, b)
    for t in TEMPS:
        got = run(z, y, k, b, t).cpu().numpy()
        ref = check(got, z, y, k, b, t, case)
        assert lay.skipped(got) == len(range(5, n * h * w, 11)) and lay.nonfinite(got) == 0
        assert lay.bins(got)[:, 0].sum() + lay.skipped(got) == n * h * w
        assert np.array_equal(lay.classes(got)[:, 0], lay.classes(ref)[:, 0])
        if case == (2, 67, 129, 5, 5, 10):                      # the same from views that start 1, 2, 3 floats into their allocation
            for offset in (1, 2, 3):
                off = run(z, y, k, b, t, offset=offset).cpu().numpy()
                assert np.array_equal(off, got), offset
        if case in R.LOOP_CASES:
            assert n * h * w > 256 * 256 and (n * h * w) % (256 * 256) != 0 and (n * h * w) % 256 != 0
    if k == 1:                                                   # conf is exactly 1 and lands in the last bin by the clamp
        assert np.array_equal(lay.bins(got)[-1], [1.0, 1.0, 1.0]) and lay.bins(got)[:-1].sum() == 0


def test_planted_uniform_logits():
    """conf is the fp32 value 1 / K, and the bin what the stated fp32 expression gives."""
    from smsut_amd import ops
    for k, b in ((3, 3), (5, 15), (7, 7), (10, 10), (32, 64)):
        z = np.full((1, 4, 5, k), 0.625, dtype=np.float32)
        y = (np.arange(20) % k).reshape(1, 4, 5).astype(np.int64)
        got = run(z, y, k, b, 1.0).cpu().numpy()
        s = np.float32(0)
        for _ in range(k):
            s = np.float32(s + np.float32(1))
        conf = np.float32(1) / s
        want_bin = min(b - 1, int(np.float32(conf * np.float32(b))))
        bins = ops.CalibrationLayout(k, b).bins(got)
        first = int((y == 0).sum())                              # the first maximum is class 0
        assert np.array_equal(bins[want_bin], [20.0, 20 * float(conf), first]), (k, b, bins, want_bin)
        assert bins[:, 0].sum() == 20
        emu, _ = R.stats(z, y, k, b, 1.0, dtype=np.float32)
        assert np.array_equal(bins, ops.CalibrationLayout(k, b).bins(emu))


def test_planted_forty_logit_lead():
    from smsut_amd import ops
    k, b = 5, 15
    z = np.zeros((1, 6, 7, k), dtype=np.float32)
    y = (np.arange(42) % k).reshape(1, 6, 7).astype(np.int64)
    np.put_along_axis(z, y[..., None], 40.0, axis=-1)
    got = run(z, y, k, b, 1.0).cpu().numpy()
    lay = ops.CalibrationLayout(k, b)
    assert np.array_equal(lay.bins(got)[-1], [42.0, 42.0, 42.0]) and lay.bins(got)[:-1].sum() == 0      # conf == 1.0f
    ref, px = R.stats(z, y, k, b, 1.0)
    tol = R.bounds(px, y, k, b, 1.0)
    cls, cls_tol = lay.classes(got), lay.classes(tol)
    print("40-logit lead: nll", cls[:, 2], "brier", cls[:, 3])
    assert (np.abs(cls[:, 2]) <= cls_tol[:, 2]).all() and (np.abs(cls[:, 3]) <= cls_tol[:, 3]).all()
    assert (np.abs(got - ref) <= tol).all()


def test_planted_nan_logit():
    from smsut_amd import ops
    k, b = 5, 10
    z, y, _ = R.draw((1, 6, 7, 5, k, b), 31)
    y = y.copy()
    y[0, 2, 3], y[0, 4, 1] = 1, 2
    base = run(z, y, k, b, 1.0).cpu().numpy()
    zn = z.copy()
    zn[0, 2, 3, 4] = np.nan                                      # not the label's channel, not the first
    zn[0, 4, 1, 0] = np.inf
    got = run(zn, y, k, b, 1.0).cpu().numpy()
    lay = ops.CalibrationLayout(k, b)
    assert lay.nonfinite(got) == 2 and lay.nonfinite(base) == 0 and lay.skipped(got) == lay.skipped(base)
    assert lay.bins(got)[:, 0].sum() == lay.bins(base)[:, 0].sum() - 2
    assert lay.classes(got)[1, 0] == lay.classes(base)[1, 0] - 1 and lay.classes(got)[2, 0] == lay.classes(base)[2, 0] - 1
    assert np.isfinite(got).all()
    y2 = y.copy()
    y2[0, 2, 3], y2[0, 4, 1] = -1, k                             # the same pixels without a label: what is left, to the bound
    check(got - np.eye(1, lay.size, lay.size - 1)[0] * 2 + np.eye(1, lay.size, lay.size - 2)[0] * 2, z, y2, k, b, 1.0, "nan")


def test_two_calls_are_bitwise_equal_and_out_is_added_to(drawn):
    for case in (R.CASES[1], R.CASES[2], *R.LOOP_CASES):
        z, y, _ = drawn[case]
        k, b = case[4:]
        for t in TEMPS:
            a = run(z, y, k, b, t)
            a2 = run(z, y, k, b, t)
            assert torch.equal(a.view(torch.int64), a2.view(torch.int64))
            z2, y2 = z[:, ::-1].copy(), y[:, ::-1].copy()
            b1 = run(z2, y2, k, b, t)
            both = run(z2, y2, k, b, t, out=a.clone())
            assert torch.equal(both.view(torch.int64), (a + b1).view(torch.int64))


def test_fit_temperature_on_the_planted_case():
    from smsut_amd.misc import utils
    z, y = R.planted(77)
    k = z.shape[-1]
    batches = [(nchw(z[i:i + 2]), torch.from_numpy(y[i:i + 2]).cuda()) for i in (0, 2)]
    t, its = utils.fit_temperature(batches, k)
    beta = R.beta_of(t)
    step, g, h = R.newton_step_size(z, y, k, beta)
    print("planted 2.5x: fitted T", t, "after", its, "iterations; fp64 |g| / h at the GPU's beta", step)
    assert its < 30 and 2.0 < t < 3.2
    assert step <= 2e-6 * beta
    raw, fit = utils.CalibrationMeter(k, 15), utils.CalibrationMeter(k, 15, temperature=t)
    for zb, yb in batches:
        raw.update(zb, yb)
        fit.update(zb, yb)
    assert fit.nll() < raw.nll() and fit.ece() < raw.ece()
    want = utils.CalibrationTotals(R.stats(z, y, k, 15, 1.0)[0], k, 15)
    assert raw.ece() == pytest.approx(want.ece(), abs=1e-6) and raw.nll() == pytest.approx(want.nll(), rel=1e-5)
    assert utils.ece(z.transpose(0, 3, 1, 2), y) == raw.ece() and utils.nll(*batches[0]) > 0
    assert utils.brier(z.transpose(0, 3, 1, 2), y) == pytest.approx(want.brier(), rel=1e-5)


def test_refusals(monkeypatch):
    from smsut_amd import _hip, ops
    from smsut_amd.misc import utils

    def boom(*a, **k):
        raise AssertionError("the device was touched")
    z = torch.zeros(2, 5, 4, 6, device="cuda").contiguous(memory_format=torch.channels_last)
    y = torch.zeros(2, 4, 6, dtype=torch.int64, device="cuda")
    out = torch.zeros(ops.CalibrationLayout(5, 15).size, dtype=torch.float64, device="cuda")
    monkeypatch.setattr(_hip, "call", boom)
    for bad in (lambda: ops.calibration_stats(z.double(), y, out), lambda: ops.calibration_stats(z, y.int(), out),
                lambda: ops.calibration_stats(z, y, out.float()), lambda: ops.calibration_stats(z.cpu(), y, out),
                lambda: ops.calibration_stats(z, y.cpu(), out), lambda: ops.calibration_stats(z, y, out.cpu()),
                lambda: ops.calibration_stats(z.cpu().numpy(), y, out), lambda: ops.calibration_stats(z, y, out, bins=15.0),
                lambda: ops.calibration_stats(z, y, out, classes="5"), lambda: ops.calibration_stats(z, y, out, temperature="1")):
        with pytest.raises(TypeError):
            bad()
    out3 = torch.zeros(ops.CalibrationLayout(3, 15).size, dtype=torch.float64, device="cuda")
    for bad in (lambda: ops.calibration_stats(z[0], y, out), lambda: ops.calibration_stats(z, y[:1], out),
                lambda: ops.calibration_stats(z, y, out[:-1]), lambda: ops.calibration_stats(z, y, out3),
                lambda: ops.calibration_stats(z, y, out.repeat(2)[::2]),
                lambda: ops.calibration_stats(z, y, out, classes=0), lambda: ops.calibration_stats(z, y, out, classes=6),
                lambda: ops.calibration_stats(z, y, out, bins=0), lambda: ops.calibration_stats(z, y, out, bins=65),
                lambda: ops.calibration_stats(z, y, out, temperature=0.0), lambda: ops.calibration_stats(z, y, out, temperature=-1.0),
                lambda: ops.calibration_stats(z, y, out, temperature=float("nan")),
                lambda: ops.calibration_stats(z, y, out, temperature=float("inf")),
                lambda: ops.calibration_stats(z, y, out, temperature=1e-40),
                lambda: utils.CalibrationMeter(5, 15, temperature=0.0), lambda: utils.CalibrationMeter(33, 15),
                lambda: utils.fit_temperature([], 5)):
        with pytest.raises(ValueError):
            bad()
    wide = torch.zeros(1, 40, 2, 2, device="cuda").contiguous(memory_format=torch.channels_last)
    with pytest.raises(ValueError):
        ops.calibration_stats(wide, y[:1, :2, :2], torch.zeros(3 * 15 + 4 * 40 + 4, dtype=torch.float64, device="cuda"))
    monkeypatch.undo()
    assert ops.calibration_stats(z[:0], y[:0], out) is out and out.abs().sum().item() == 0      # N == 0: nothing is launched
    lib = _hip.load()
    assert lib.smsut_calibration_ws(1, 1, 1, 40, 33, 15) == -1 and lib.smsut_calibration_ws(1, 1, 1, 5, 5, 65) == -1
    assert lib.smsut_calibration_ws(65536, 1, 1, 5, 5, 15) == -1 and lib.smsut_calibration_ws(1, 16385, 1, 5, 5, 15) == -1
    assert lib.smsut_calibration_ws(2, 4, 6, 5, 5, 15) == (3 * 15 + 4 * 5 + 4) * 8
