"""Host side of the volume preparation (no device): the oracle of tests/volume_ref.py against scipy, ``resample_plan`` against
hand-worked cases, ``write_slices`` read back through ``BalanceDataset``, and the argument checks that come before any launch."""
import os

import numpy as np
import pytest
import torch

import volume_ref as R


def test_oracle_matches_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for shape in ((5, 7, 33), (1, 6, 9), (2, 3, 70), (3, 2, 2)):
        v = R.volume(shape, 5)
        want = v.astype(np.float64)
        for ax in range(3):
            if shape[ax] > 1:
                want = ndi.spline_filter1d(want, 3, axis=ax, mode="mirror")
        got = R.coefficients(v)
        assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max(), shape
    coef = np.random.default_rng(3).standard_normal((9, 40, 37))
    for out_size, num, den, start, off in (((13, 24, 24), (9, 40, 37), (20, 31, 37), (0, 3, 5), (0, 0, 0)),
                                           ((9, 30, 37), (20, 31, 37), (9, 40, 37), (0, 0, 0), (0, 3, 5))):
        got, ok = R.resample(coef, out_size, num, den, start, off)
        grid = np.meshgrid(*(R.coords(out_size[a], start[a], num[a], den[a], off[a]) for a in range(3)), indexing="ij")
        want = ndi.map_coordinates(coef, grid, order=3, mode="mirror", prefilter=False)
        assert np.abs(got - np.where(ok, want, 0.0)).max() <= 1e-13
        assert (got[~ok] == 0.0).all()


def test_oracle_interpolates_and_ref32_is_close():
    v = R.volume((4, 9, 11), 2)
    c = R.coefficients(v)
    back, ok = R.resample(c, v.shape, v.shape, v.shape, (0, 0, 0))
    assert ok.all() and np.abs(back - v).max() <= 1e-11 * np.abs(v).max()
    c32 = R.coefficients(v, np.float32)
    assert c32.dtype == np.float32 and 0 < R.bar(c32, c) <= 16 * 27 * 2.0 ** -23 * np.abs(c).max()
    assert R.mirror([-1, 0, 4, 5, 6, -9], 5).tolist() == [1, 0, 4, 3, 2, 1] and R.mirror([-3, 7], 1).tolist() == [0, 0]


def test_oracle_nearest_rounds_halves_up_and_window_truncates():
    lab = np.arange(2 * 3 * 8, dtype=np.uint8).reshape(2, 3, 8)
    out = R.nearest(lab, (2, 3, 16), (1, 1, 1), (1, 1, 2), (0, 0, 0))          # x = i / 2: every odd i is a tie
    assert out[0, 0].tolist() == [0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 0]     # i = 15: x = 7.5 is outside
    lut = R.chaos_lut()
    assert lut[[0, 54, 55, 70, 71, 110, 135, 175, 200, 239, 240, 255]].tolist() == [0, 0, 1, 1, 0, 2, 2, 3, 3, 0, 4, 4]
    v = np.array([-5.0, 0.0, 0.999, 1.0, 50.0, 99.9, 100.0, 200.0], dtype=np.float32)
    assert R.window(v, 0.0, 100.0).tolist() == [0, 0, 2, 2, 127, 254, 255, 255]
    assert R.window(v, 3.0, 3.0).tolist() == [0] * 8


def test_resample_plan_hand_worked():
    from smsut_amd.data_pprocess import volume as V
    p = V.resample_plan((30, 256, 256), (7.7, 1.89, 1.89))
    # z: 30 * 7.7 / 5 = 46.2 -> 46; in plane: 256 * 1.89 / 1.5 = 322.56 -> 322; start = (322 - 256) // 2 = 33
    assert p.new_size == (46, 322, 322) and p.start == (0, 33, 33) and p.out_size == (46, 256, 256)
    assert p.spacing == (7.7 * 30 / 46, 1.89 * 256 / 322, 1.89 * 256 / 322)
    assert abs(p.spacing[0] - 5.0217391) < 1e-6 and abs(p.spacing[1] - 1.5026087) < 1e-6
    # in-plane size below the crop: 100 * 1.5 / 1.5 = 100 -> 256 (2.56x up), 120 -> 256 (2.13x up); the spacing shrinks with it
    q = V.resample_plan((20, 100, 120), (5.0, 1.5, 1.5))
    assert q.new_size == (20, 256, 256) and q.start == (0, 0, 0) and q.out_size == (20, 256, 256)
    assert q.spacing == (5.0, 1.5 * 100 / 256, 1.5 * 120 / 256)
    # more than 2x up: the samples past old - 0.5 are outside.  x = i * 100 / 256 < 99.5  <=>  i <= 254
    x = R.coords(256, 0, 100, 256)
    assert R.inside(x, 100).sum() == 255 and not R.inside(x, 100)[255]
    r = V.resample_plan((40, 512, 512), (3.0, 0.8, 0.8), new_spacing=(5, 1.5, 1.5), crop_size=256)
    assert r.new_size == (24, 273, 273) and r.start == (0, 8, 8)
    with pytest.raises(ValueError):
        V.resample_plan((3, 256, 256), (1.0, 1.5, 1.5))                          # int(3 * 1 / 5) == 0 slices


def test_argument_validation():
    from smsut_amd import ops
    from smsut_amd.data_pprocess import volume as V
    for bad in ((0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf")), (1.0, 1.0)):
        with pytest.raises(ValueError):
            V.resample_plan((30, 256, 256), bad)
        with pytest.raises(ValueError):
            V.resample_plan((30, 256, 256), (1.0, 1.0, 1.0), new_spacing=bad)
    for size in ((0, 256, 256), (30, 4097, 256), (30, 256), (4096, 4096, 4096)):
        with pytest.raises(ValueError):
            V.resample_plan(size, (5.0, 1.5, 1.5))
    with pytest.raises(ValueError):
        V.resample_plan((4096, 300, 300), (5.0, 1.5, 1.5), new_spacing=(1.0, 1.5, 1.5))      # new_z = 20480
    with pytest.raises(ValueError):
        V.resample_plan((30, 256, 256), (5.0, 1.5, 1.5), crop_size=0)
    f, u = torch.zeros(2, 3, 4), torch.zeros(2, 3, 4, dtype=torch.uint8)
    one = ((1, 1, 1),) * 2 + ((0, 0, 0),)
    # argument errors come first, as ValueError, with CPU tensors as well: the device is not touched
    for call in (lambda: ops.bspline_coefficients(u), lambda: ops.bspline_coefficients(f[0]),
                 lambda: ops.resample_volume(f, (0, 3, 4), *one), lambda: ops.resample_volume(f, (2, 3, 4097), *one),
                 lambda: ops.resample_volume(f, (2, 3, 4), (1, 1, 0), (1, 1, 1), (0, 0, 0)),
                 lambda: ops.resample_volume(f, (2, 3, 4), (1, 1, 1), (1, 1, 1), (0, -1, 0)),
                 lambda: ops.resample_volume(f, (2, 3, 4), (1, 1), (1, 1, 1), (0, 0, 0)),
                 lambda: ops.resample_labels(f, (2, 3, 4), *one), lambda: ops.resample_labels(u, (2, 3, 4), *one, lut=u),
                 lambda: ops.order_statistics(f, []), lambda: ops.order_statistics(f, [24]), lambda: ops.order_statistics(f, [-1]),
                 lambda: ops.order_statistics(f, list(range(9))), lambda: ops.order_statistics(u, [0]),
                 lambda: ops.order_statistics(f[:0], [0]),
                 lambda: ops.window_u8(u, torch.zeros(2)), lambda: ops.window_u8(f, torch.zeros(3)),
                 lambda: ops.window_u8(f, torch.zeros(2, dtype=torch.float64))):
        with pytest.raises(ValueError):
            call()
    if not torch.cuda.is_available():
        from smsut_amd import _hip
        for call in (lambda: ops.bspline_coefficients(f), lambda: ops.resample_volume(f, (2, 3, 4), *one),
                     lambda: ops.resample_labels(u, (2, 3, 4), *one), lambda: ops.order_statistics(f, [0, 23]),
                     lambda: ops.window_u8(f, torch.zeros(2))):
            with pytest.raises(_hip.SmsutHipError):                               # valid arguments, CPU tensors: refused, no fallback
                call()
    with pytest.raises(ValueError):
        V.write_slices(np.zeros((2, 4, 4), np.uint8), np.zeros((2, 4, 5), np.uint8), "/nonexistent", "t2", "001")
    with pytest.raises(ValueError):
        V.write_slices(np.zeros((2, 4, 4), np.float32), np.zeros((2, 4, 4), np.uint8), "/nonexistent", "t2", "001")


def test_workspace_queries_reject_invalid_sizes():
    import ctypes
    from smsut_amd import _hip as H
    lib = H.load()
    assert lib.smsut_bspline_ws(3, 5, 7) == 3 * 5 * 7 * 4 and lib.smsut_bspline_ws(0, 5, 7) == -1
    assert lib.smsut_bspline_ws(4096, 4096, 4096) == -1 and lib.smsut_bspline_ws(1, 1, 4097) == -1
    assert lib.smsut_resample_ws(13, 24, 24) > 0 and lib.smsut_resample_ws(13, 0, 24) == -1
    ws = lib.smsut_order_statistics_ws
    assert ws(1, 1) > 0 and ws(ctypes.c_int64(2 ** 31 - 1), 8) > 0
    assert ws(0, 1) == -1 and ws(ctypes.c_int64(2 ** 31), 1) == -1 and ws(10, 0) == -1 and ws(10, 9) == -1


def test_write_slices_round_trips_through_the_dataset(tmp_path):
    from smsut_amd.data_loader.inTurnLoader import BalanceDataset
    from smsut_amd.data_pprocess import volume as V
    rng = np.random.default_rng(8)
    vols = {}
    for modality, pid, shape in (("t2", "007", (5, 16, 12)), ("ct", "012", (3, 16, 12)), ("t2", "031", (12, 16, 12))):
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        lab = rng.integers(0, 5, size=shape, dtype=np.uint8)
        root = V.write_slices(torch.from_numpy(img), lab, str(tmp_path), modality, pid)
        assert set(os.listdir(root)) == {"images", "labels", f"{modality}_{pid}.npy"}
        assert sorted(os.listdir(os.path.join(root, "images")))[-1] == f"{modality}_{pid}_{shape[0] - 1:03d}.png"
        assert np.array_equal(np.load(os.path.join(root, f"{modality}_{pid}.npy")), lab)
        vols[(modality, pid)] = (img, lab)
    with open(tmp_path / "split.yaml", "w") as f:
        f.write("ct:\n  test: ['012']\nt1in:\n  test: []\nt1out:\n  test: []\nt2:\n  test: ['007', '031']\n")
    ds = BalanceDataset(str(tmp_path), "test", 0, "split.yaml")
    order = [("ct", "012"), ("t2", "007"), ("t2", "031")]                       # modalities in config order, pids as listed
    assert len(ds) == sum(vols[k][0].shape[0] for k in order)
    assert ds.images.dtype == torch.uint8 and ds.labels.dtype == torch.uint8
    assert ds.images.numpy().tobytes() == np.concatenate([vols[k][0] for k in order]).tobytes()
    assert ds.labels.numpy().tobytes() == np.concatenate([vols[k][1] for k in order]).tobytes()
    assert ds.names[0] == "ct_012_000" and ds.names[-1] == "t2_031_011"
