"""Sliding-window inference on the device: ``ops.window_blend`` (csrc/window.hip) against tests/window_ref.py, the exact
properties of the blend, ``Predictor.predict_windows``, ``prepare_volume(field_of_view='full')``, ``predict_volume`` and the command
line.

1. the kernel against the fp64 blend at the cases of window_ref.CASES: ``prob`` and ``conf`` within ``budget(cover)``, ``pred`` equal
   wherever the reference's gap is at least 4 budgets, the share of pixels left out asserted (at most 0.5 %);
2. exact: one tile and disjoint tiles pass through bit for bit, planted labels come back, two calls agree bitwise, bad plans raise
   before any launch;
3. the predictor on a pointwise stub (labels exactly those of the stub on the whole image) and on a small U-Net against
   ``tta_ref.merge_ref`` per tile followed by ``window_ref.blend_ref``, fed the very logits the predictor merged;
4. the full field of view: its central window is the cropped output bit for bit, ``predict_volume`` is the composition of its
   pieces and labels voxels outside the crop, and the command line writes the same files."""
import numpy as np
import pytest
import torch

import tta_ref as T
import window_ref as R

pytestmark = pytest.mark.gpu

C = 5
A = (0.0, 3.1, -2.3, 1.7, -0.9)
B2 = (0.4, -1.9, 2.2, -3.3, 1.1)
SH = (0.3, -0.2, 0.55, -0.7, 0.1)


@pytest.fixture(scope="module")
def dev():
    import smsut_amd  # noqa: F401
    return torch.device("cuda")


def stub(x):
    """The pointwise network of tests/test_predict_gpu.py: [B, 1, H, W] -> logits [B, C, H, W] in NHWC memory,
    z_c = a_c x + b_c x^2 + s_c of the pixel's own value (its class gap is above 1e-3 at all 256 intensities)."""
    v = x.permute(0, 2, 3, 1)
    a, b, s = (torch.tensor(t, device=x.device) for t in (A, B2, SH))
    return (v * a + v * v * b + s).contiguous().permute(0, 3, 1, 2)


def loader_float(u8):
    return u8.float().div(255).sub(.5).div(.5)


def on_device(tile, dev, offset):
    """The tile on the device; ``offset``: as a contiguous view that starts one float past its (16-byte aligned) allocation."""
    if not offset:
        return tile.to(dev)
    buf = torch.empty(tile.numel() + 1, dtype=torch.float32, device=dev)
    view = buf[1:].view(tile.shape)
    view.copy_(tile)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("idx", range(len(R.CASES)), ids=R.IDS)
def test_blend_against_fp64(dev, idx):
    from smsut_amd import ops
    c = R.cases()[idx]
    tiles = [on_device(t, dev, c.offset) for t in c.tiles]
    wy, wx = ops.window_weights(c.window, c.blend, dev), ops.window_weights(c.window, c.blend, dev)
    assert np.array_equal(wy.cpu().numpy(), c.wy) and ops.window_plan(c.h, c.window, c.overlap) == c.ys
    pred, conf, prob = ops.window_blend(tiles, c.ys, c.xs, (c.h, c.w), wy, wx, want_conf=True, want_prob=True)
    torch.cuda.synchronize()
    eprob = float((prob.cpu().double() - c.prob).abs().max())
    econf = float((conf.cpu().double() - c.conf).abs().max())
    decided = c.gap >= 4 * c.budget
    left_out = float((~decided).double().mean())
    print(f"window_blend {R.IDS[idx]}: {len(c.ys)} x {len(c.xs)} tiles, cover {c.cover}, max |prob - ref| = {eprob:.3e}, "
          f"max |conf - ref| = {econf:.3e}, B = {c.budget:.3e}, left out = {left_out:.4%}, smallest gap = {float(c.gap.min()):.3e}")
    assert pred.dtype == torch.uint8 and tuple(pred.shape) == (c.n, c.h, c.w) and tuple(prob.shape) == (c.n, c.h, c.w, c.k)
    assert eprob <= c.budget and econf <= c.budget
    assert left_out <= 0.005
    assert torch.equal(pred.cpu().long()[decided], c.pred[decided])
    assert torch.equal(conf, prob.gather(-1, pred.long().unsqueeze(-1)).squeeze(-1))             # conf is prob at pred, to the bit


def test_one_tile_passes_through(dev):
    from smsut_amd import ops
    g = torch.Generator().manual_seed(11)
    p = torch.softmax(3 * torch.randn(2, 17, 17, C, generator=g), dim=-1)
    p[0, 3, 4] = torch.tensor([0.3, 0.3, 0.1, 0.3, 0.0])                                         # a tie: the first maximum wins
    tile = p.to(dev)
    w = ops.window_weights(17, "gaussian", dev)
    pred, conf, prob = ops.window_blend([tile], (0,), (0,), (17, 17), w, w, want_conf=True, want_prob=True)
    assert torch.equal(prob, tile)
    assert torch.equal(pred.cpu().long(), R.first_max(p)) and int(pred[0, 3, 4]) == 0
    assert torch.equal(conf, tile.max(dim=-1).values)


def test_disjoint_tiles_are_copied(dev):
    from smsut_amd import ops
    g = torch.Generator().manual_seed(12)
    full = torch.softmax(3 * torch.randn(2, 40, 48, C, generator=g), dim=-1).to(dev)
    ys, xs = ops.window_plan(40, 20, 0.0), ops.window_plan(48, 24, 0.0)
    assert ys == (0, 20) and xs == (0, 24)
    tiles = [full[:, y0:y0 + 20, x0:x0 + 24].contiguous() for y0 in ys for x0 in xs]
    wy, wx = ops.window_weights(20, "gaussian", dev), ops.window_weights(24, "gaussian", dev)
    pred, conf, prob = ops.window_blend(tiles, ys, xs, (40, 48), wy, wx, want_conf=True, want_prob=True)
    assert torch.equal(prob, full)                                                               # every pixel under one tile
    assert torch.equal(conf, full.max(dim=-1).values) and torch.equal(pred.long(), R.first_max(full.cpu()).to(dev))


def test_planted_labels_come_back(dev):
    """Tiles cut from 8 onehot(L) + noise of a label map with no symmetry: a swapped origin or a swapped axis moves labels."""
    from smsut_amd import ops
    n, h, w, win = 2, 37, 50, 16
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    lab = np.stack([(yy // 3 + 2 * (xx // 5) + s) % C for s in range(n)])                        # [n, h, w]: differs under flips, swaps
    assert not np.array_equal(lab[:, :, :h], np.swapaxes(lab[:, :, :h], 1, 2)) and not np.array_equal(lab, lab[:, ::-1])
    full = 8.0 * np.eye(C, dtype=np.float32)[lab] + np.random.default_rng(13).random((n, h, w, C), dtype=np.float32)
    full = torch.from_numpy(full).to(dev)
    ys, xs = ops.window_plan(h, win, 0.5), ops.window_plan(w, win, 0.5)
    tiles = [full[:, y0:y0 + win, x0:x0 + win].contiguous() for y0 in ys for x0 in xs]
    wt = ops.window_weights(win, "gaussian", dev)
    pred, _, prob = ops.window_blend(tiles, ys, xs, (h, w), wt, wt, want_prob=True)
    assert torch.equal(pred.cpu().long(), torch.from_numpy(lab).long())
    assert float((prob - full).abs().max()) <= 9.0 * R.budget(9)                                 # identical tiles: the blend is the tile


def test_two_calls_are_bitwise_equal(dev):
    from smsut_amd import ops
    c = R.cases()[0]
    tiles = [t.to(dev) for t in c.tiles]
    wt = ops.window_weights(c.window, c.blend, dev)
    a = ops.window_blend(tiles, c.ys, c.xs, (c.h, c.w), wt, wt, want_conf=True, want_prob=True)
    b = ops.window_blend(tiles, c.ys, c.xs, (c.h, c.w), wt, wt, want_conf=True, want_prob=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    only_pred = ops.window_blend(tiles, c.ys, c.xs, (c.h, c.w), wt, wt)                          # the optional outputs do not change it
    assert only_pred[1] is None and only_pred[2] is None and torch.equal(only_pred[0], a[0])


def test_bad_plans_raise_without_a_launch(dev, monkeypatch):
    from smsut_amd import _hip, ops
    lib = _hip.load()
    entered = []
    monkeypatch.setattr(lib, "smsut_window_blend", lambda *a: entered.append(a) or 0)
    wt = ops.window_weights(8, "gaussian", dev)
    t = torch.zeros(1, 8, 8, 2, device=dev)
    ys, xs = ops.window_plan(32, 8, 0.75), ops.window_plan(16, 8, 0.75)
    assert len(ys) * len(xs) == 65
    with pytest.raises(ValueError, match="at most 64"):
        ops.window_blend([t] * 65, ys, xs, (32, 16), wt, wt)
    with pytest.raises(ValueError, match="uncovered"):
        ops.window_blend([t, t], (0, 10), (0,), (18, 8), wt, wt)
    with pytest.raises(ValueError, match="contiguous"):
        ops.window_blend([torch.zeros(1, 8, 8, 4, device=dev)[..., :2]], (0,), (0,), (8, 8), wt, wt)
    with pytest.raises(ValueError):
        ops.window_blend([t], (0,), (0,), (8, 8), wt.cpu(), wt)                                  # a table on another device
    with pytest.raises(TypeError):
        ops.window_blend([t.cpu()], (0,), (0,), (8, 8), wt, wt)
    assert entered == []
    monkeypatch.undo()
    # ... and the C ABI itself refuses a tile outside the grid and 65 tiles (status -1, nothing launched)
    import ctypes
    ptrs = (ctypes.c_void_p * 65)(*[t.data_ptr()] * 65)
    one = (ctypes.c_int * 1)(1)
    many = (ctypes.c_int * 65)(*range(65))
    pred = torch.zeros(1, 8, 8, dtype=torch.uint8, device=dev)
    with pytest.raises(_hip.SmsutHipError, match="invalid argument"):
        _hip.call("smsut_window_blend", ctypes.addressof(ptrs), ctypes.addressof(one), ctypes.addressof(one), wt, wt, pred, None, None,
                  1, 1, 1, 8, 8, 8, 8, 2, _hip.stream_ptr())
    with pytest.raises(_hip.SmsutHipError, match="invalid argument"):
        _hip.call("smsut_window_blend", ctypes.addressof(ptrs), ctypes.addressof(many), ctypes.addressof(one), wt, wt, pred, None, None,
                  65, 1, 1, 8, 8, 8, 8, 2, _hip.stream_ptr())
    torch.cuda.synchronize()
    assert int(pred.sum()) == 0


@pytest.mark.parametrize("tta", ["none", "flips"])
def test_predict_windows_on_the_stub(dev, tta):
    from smsut_amd import ops
    from smsut_amd.predict import Predictor
    img = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (4, 40, 52), dtype=np.uint8)).to(dev)
    logits = stub(loader_float(img).unsqueeze(1))
    p = Predictor(stub, batch_size=3, tta=tta)                                                   # two groups, the last padded
    pred, conf = p.predict_windows(img, 24, confidence=True)
    assert pred.dtype == torch.uint8 and pred.shape == img.shape
    assert torch.equal(pred.long(), ops.argmax_channels(logits))
    ref_conf = torch.softmax(logits.double(), dim=1).max(dim=1).values
    t = len(ops.tta_transforms(tta))
    bound = T.budget(C, t) + R.budget(9)                                                         # 3 x 4 tiles, cover 9
    err = float((conf.double() - ref_conf).abs().max())
    print(f"predict_windows stub {tta}: max |conf - fp64 softmax maximum| = {err:.3e}, bound = {bound:.3e}")
    assert err <= bound
    only, none_conf = p.predict_windows(img, 24)
    assert none_conf is None and torch.equal(only, pred)
    for blend, overlap in (("constant", 0.5), ("gaussian", 0.25)):
        again, _ = p.predict_windows(img, 24, overlap=overlap, blend=blend)
        assert torch.equal(again, pred)


def test_one_window_is_predict_slices(dev):
    from smsut_amd.predict import Predictor
    img = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (5, 24, 24), dtype=np.uint8)).to(dev)
    for tta, temperature in (("none", None), ("d4", None), ("flips", 1.7)):
        p = Predictor(stub, batch_size=2, tta=tta, temperature=temperature)
        a, b = p.predict_windows(img, 24, confidence=True), p.predict_slices(img, confidence=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), tta


def small_unet(seed, dev):
    from smsut_amd.network.unet import UNet
    torch.manual_seed(seed)
    return UNet(1, C, 8, norm_type="instance", act_type="lrelu").to(dev).eval()


def test_real_network_against_fp64(dev):
    from smsut_amd import ops
    from smsut_amd.predict import Predictor
    net = small_unet(21, dev)
    seen = []

    def recording(x):
        out = net(x)
        seen.append(out)
        return out
    img = torch.from_numpy(np.random.default_rng(8).integers(0, 256, (4, 48, 48), dtype=np.uint8)).to(dev)
    tr = ops.tta_transforms("flips")
    pred, conf = Predictor(recording, batch_size=4, tta="flips").predict_windows(img, 32, confidence=True)
    ys = xs = ops.window_plan(48, 32, 0.5)
    assert ys == (0, 16) and len(seen) == 4 * len(tr)
    tiles = []
    for i in range(4):                                                                           # per tile: the members the predictor merged
        members = [z.permute(0, 2, 3, 1).cpu() for z in seen[i * len(tr):(i + 1) * len(tr)]]
        tiles.append(T.merge_ref(members, tr)[2])                                                # fp64 mean probabilities [N, 32, 32, C]
    wt = R.weights(32, "gaussian")
    rpred, rconf, _, rgap, cover = R.blend_ref(tiles, ys, xs, (48, 48), wt, wt)
    b = T.budget(C, len(tr)) + R.budget(cover)
    decided = rgap >= 4 * b
    left_out = float((~decided).double().mean())
    err = float((conf.cpu().double() - rconf).abs().max())
    print(f"U-Net x flips, 2 x 2 windows: cover {cover}, pixels left out = {left_out:.4%}, smallest gap = {float(rgap.min()):.3e}, "
          f"max |conf - ref| = {err:.3e}, B = {b:.3e}, classes predicted = {torch.unique(rpred).tolist()}")
    assert cover == 4 and left_out <= 0.005
    assert torch.equal(pred.cpu().long()[decided], rpred[decided])
    assert err <= b
    first = loader_float(img[:, :32, :32]).unsqueeze(1).contiguous()                             # tile (0, 0), member 0: the crop itself
    assert torch.equal(seen[0], net(first))


def synthetic_ct():
    """The 12 x 40 x 44 volume of tests/test_predict_gpu.py::test_predict_volume_is_the_composition_of_its_pieces."""
    rng = np.random.default_rng(4)
    zz, yy, xx = np.meshgrid(np.arange(12), np.arange(40), np.arange(44), indexing="ij")
    return (500.0 * np.sin(yy / 5.0 + zz / 3.0) * np.cos(xx / 6.0) - 300.0 + 30.0 * rng.standard_normal((12, 40, 44))).astype(np.float32)


SPACING = (5.0, 1.25, 1.25)                                     # -> a 12 x 33 x 36 grid; the crop is its central 32 x 32


def test_full_field_of_view_contains_the_crop(dev):
    from smsut_amd.data_pprocess.volume import ResamplePlan, prepare_volume
    vol = synthetic_ct()
    lab = (np.random.default_rng(9).integers(0, 5, vol.shape)).astype(np.uint8)
    crop_img, crop_lab, crop = prepare_volume(vol, lab, SPACING, "ct", crop_size=32)
    full_img, full_lab, full = prepare_volume(vol, lab, SPACING, "ct", crop_size=32, field_of_view="full")
    assert crop.new_size == (12, 33, 36) and crop.start == (0, 0, 2) and crop.out_size == (12, 32, 32)
    assert full == ResamplePlan(crop.new_size, crop.spacing, (0, 0, 0), crop.new_size)
    assert tuple(full_img.shape) == (12, 33, 36) and full_img.dtype == torch.uint8 and tuple(full_lab.shape) == (12, 33, 36)
    (_, sy, sx) = crop.start
    assert torch.equal(full_img[:, sy:sy + 32, sx:sx + 32], crop_img)                            # the same index map, the same bounds
    assert torch.equal(full_lab[:, sy:sy + 32, sx:sx + 32], crop_lab)
    again = prepare_volume(vol, lab, SPACING, "ct", crop_size=32, field_of_view="crop")
    assert torch.equal(again[0], crop_img) and again[2] == crop


def test_predict_volume_full_is_the_composition_of_its_pieces(dev):
    from smsut_amd import config as cfg, ops
    from smsut_amd.data_pprocess.volume import prepare_volume, restore_labels
    from smsut_amd.predict import Predictor, predict_volume
    vol = synthetic_ct()
    p = Predictor(stub, batch_size=5, tta="none")
    res = predict_volume(p, vol, SPACING, "ct", crop_size=32, confidence=True, field_of_view="full")
    image_u8, _, plan = prepare_volume(vol, None, SPACING, "ct", crop_size=32, field_of_view="full")
    assert plan == res.plan and plan.out_size == (12, 33, 36)
    raw, conf = p.predict_windows(image_u8, 32, confidence=True)
    cleaned = ops.cc_filter(raw, cfg.n_modal, per_slice=False)
    assert torch.equal(res.labels_processed, cleaned) and torch.equal(res.confidence, conf)
    assert torch.equal(res.labels, restore_labels(cleaned, plan, vol.shape))
    assert tuple(res.labels.shape) == vol.shape and res.labels.dtype == torch.uint8
    assert torch.equal(raw.long(), ops.argmax_channels(stub(loader_float(image_u8).unsqueeze(1))))   # (the stub is pointwise)
    other = predict_volume(p, vol, SPACING, "ct", crop_size=32, cleanup=False, field_of_view="full", overlap=0.25, blend="constant")
    assert other.confidence is None and torch.equal(other.labels_processed, raw)
    # outside the crop's footprint: labelled by "full", zero by "crop"
    full = predict_volume(p, vol, SPACING, "ct", crop_size=32, cleanup=False, field_of_view="full")
    crop = predict_volume(p, vol, SPACING, "ct", crop_size=32, cleanup=False)
    outside = restore_labels(torch.ones(crop.plan.out_size, dtype=torch.uint8, device=dev), crop.plan, vol.shape) == 0
    assert int(outside.sum()) > 0
    assert int(crop.labels[outside].max()) == 0 and int((full.labels[outside] != 0).sum()) >= 1
    assert torch.equal(full.labels[~outside], crop.labels[~outside])                             # inside it the two agree (pointwise stub)
    with pytest.raises(ValueError, match="uncertainty"):
        predict_volume(p, vol, SPACING, "ct", crop_size=32, uncertainty=True, field_of_view="full")


def test_full_equals_crop_when_the_grid_is_the_crop(dev):
    from smsut_amd.predict import Predictor, predict_volume
    vol = synthetic_ct()[:, :32, :32].copy()
    spacing = (5.0, 1.5, 1.5)                                   # the resampled grid is 12 x 32 x 32: the crop itself
    p = Predictor(stub, batch_size=5, tta="flips")
    a = predict_volume(p, vol, spacing, "ct", crop_size=32, confidence=True)
    b = predict_volume(p, vol, spacing, "ct", crop_size=32, confidence=True, field_of_view="full")
    assert a.plan == b.plan and a.plan.out_size == (12, 32, 32)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


def test_cli_writes_the_full_field_of_view(dev, tmp_path, monkeypatch):
    from smsut_amd import config as cfg
    from smsut_amd import predict as P
    from smsut_amd.network.unet import UNet
    monkeypatch.setattr(cfg, "expr_root", str(tmp_path / "runs"))
    ckpt = tmp_path / "runs" / "UnetTrainer" / "000" / "ckpt"
    ckpt.mkdir(parents=True)
    torch.manual_seed(31)
    net = UNet(cfg.img_channels, cfg.n_label + 1, cfg.base_width, norm_type="instance", act_type="lrelu")
    torch.save({k: v.contiguous() for k, v in net.state_dict().items()}, ckpt / "last.ckpt")
    vol = (np.random.default_rng(6).standard_normal((2, 280, 264)) * 200.0).astype(np.float32)
    np.save(tmp_path / "scan.npy", vol)
    out = tmp_path / "out"
    P.main(["--trainer", "unet", "-i", "000", "--image", str(tmp_path / "scan.npy"), "--spacing", "5.0", "1.5", "1.5",
            "--modality", "ct", "--confidence", "--field-of-view", "full", "--overlap", "0.25", "--out", str(out)])
    labels, proc, conf = (np.load(out / f) for f in ("labels.npy", "labels_processed.npy", "confidence.npy"))
    assert labels.shape == vol.shape and labels.dtype == np.uint8
    assert proc.shape == (2, 280, 264) and conf.shape == proc.shape and conf.dtype == np.float32
    net.load_state_dict(torch.load(ckpt / "last.ckpt", map_location="cpu"))
    ref = P.predict_volume(P.Predictor(net.to(dev), classes=cfg.n_label + 1), vol, (5.0, 1.5, 1.5), "ct", confidence=True,
                           field_of_view="full", overlap=0.25)
    assert np.array_equal(labels, ref.labels.cpu().numpy())
    assert np.array_equal(proc, ref.labels_processed.cpu().numpy())
    assert np.array_equal(conf, ref.confidence.cpu().numpy())
