"""``smsut_amd.predict``: ``Predictor``, ``predict_volume`` and the command line, on the device.

1. a pointwise stub network (logits = a fixed function of the pixel's own intensity) is exactly D4-equivariant: every transform
   set must return the un-augmented prediction, and the confidence the single-member probability within tta_ref.budget;
2. ``predict_volume`` is bitwise the composition of the existing pieces called by hand;
3. a real U-Net (random weights) under 'd4', and two U-Nets under 'flips', against ``tta_ref.merge_ref`` fed the very logits the
   predictor merged, under the gap rule of tests/test_tta_gpu.py (at most 0.5 % of the pixels left out, asserted);
4. the command line writes its files and ``labels.npy`` equals ``predict_volume``'s."""
import types

import numpy as np
import pytest
import torch

import tta_ref as R

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
    """[B, 1, H, W] -> logits [B, C, H, W] in NHWC memory: z_c = a_c x + b_c x^2 + s_c, elementwise in the pixel's own value."""
    v = x.permute(0, 2, 3, 1)                                   # [B, H, W, 1]
    a, b, s = (torch.tensor(t, device=x.device) for t in (A, B2, SH))
    return (v * a + v * v * b + s).contiguous().permute(0, 3, 1, 2)


def loader_float(u8):
    return u8.float().div(255).sub(.5).div(.5)


def test_stub_network_is_equivariant(dev):
    from smsut_amd import ops
    from smsut_amd.predict import Predictor
    bs, h = 3, 20
    table = stub(loader_float(torch.arange(256, dtype=torch.uint8, device=dev)).view(1, 1, 16, 16))
    top2 = torch.topk(table.double(), 2, dim=1).values
    assert float((top2[:, 0] - top2[:, 1]).min()) > 1e-3       # (the stub itself: no intensity sits on a class boundary)
    img = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (bs + 1, h, h), dtype=np.uint8)).to(dev)
    before = ops.layout_copies()
    base, none_conf = Predictor(stub, batch_size=bs, tta="none").predict_slices(img)
    assert none_conf is None and base.dtype == torch.uint8 and base.shape == img.shape
    assert torch.equal(base.long(), ops.argmax_channels(stub(loader_float(img).unsqueeze(1))))
    ref_conf = torch.softmax(stub(loader_float(img).unsqueeze(1)).double(), dim=1).max(dim=1).values
    for tta in ("flips", "d4", "none"):
        pred, conf = Predictor(stub, batch_size=bs, tta=tta).predict_slices(img, confidence=True)
        assert torch.equal(pred, base), tta
        t = len(ops.tta_transforms(tta))
        err = float((conf.double() - ref_conf).abs().max())
        print(f"stub {tta}: max |conf - single-member probability| = {err:.3e}, B = {R.budget(C, t):.3e}")
        assert err <= R.budget(C, t), tta
    assert ops.layout_copies() == before                        # the members were merged in place
    two, _ = Predictor([stub, stub], batch_size=bs, tta="flips").predict_slices(img)          # an ensemble of T = 8
    assert torch.equal(two, base)
    with pytest.raises(ValueError):                             # a quarter turn of a non-square slice, before any launch
        Predictor(stub, batch_size=bs, tta="d4").predict_slices(img[:, :, :18].contiguous())


def test_predict_volume_is_the_composition_of_its_pieces(dev):
    from smsut_amd import config as cfg, ops
    from smsut_amd.data_pprocess.volume import prepare_volume, restore_labels
    from smsut_amd.predict import Predictor, predict_volume
    rng = np.random.default_rng(4)
    zz, yy, xx = np.meshgrid(np.arange(12), np.arange(40), np.arange(44), indexing="ij")
    vol = (500.0 * np.sin(yy / 5.0 + zz / 3.0) * np.cos(xx / 6.0) - 300.0 + 30.0 * rng.standard_normal((12, 40, 44))).astype(np.float32)
    spacing = (5.0, 1.25, 1.25)                                 # -> a 12 x 33 x 36 grid, cropped to 32 x 32 in plane
    p = Predictor(stub, batch_size=5, tta="none")
    res = predict_volume(p, vol, spacing, "ct", crop_size=32)
    image_u8, _, plan = prepare_volume(vol, None, spacing, "ct", crop_size=32)
    assert plan.out_size == (12, 32, 32) and plan == res.plan
    raw = ops.argmax_channels(stub(loader_float(image_u8).unsqueeze(1))).to(torch.uint8)
    cleaned = ops.cc_filter(raw, cfg.n_modal, per_slice=False)
    assert torch.equal(res.labels_processed, cleaned)
    assert torch.equal(res.labels, restore_labels(cleaned, plan, vol.shape))
    assert tuple(res.labels.shape) == vol.shape and res.labels.dtype == torch.uint8 and res.confidence is None
    assert len(torch.unique(raw)) >= 3                          # (the volume exercises several classes)
    # stage by stage
    r0 = predict_volume(p, vol, spacing, "ct", crop_size=32, cleanup=False, restore=False)
    assert torch.equal(r0.labels_processed, raw) and torch.equal(r0.labels, raw)
    r1 = predict_volume(p, vol, spacing, "ct", crop_size=32, cleanup=True, restore=False, confidence=True)
    assert torch.equal(r1.labels, cleaned) and tuple(r1.confidence.shape) == (12, 32, 32)
    r2 = predict_volume(p, vol, spacing, "ct", crop_size=32, cleanup=False, restore=True)
    assert torch.equal(r2.labels, restore_labels(raw, plan, vol.shape)) and torch.equal(r2.labels_processed, raw)


def small_unet(seed, dev):
    from smsut_amd.network.unet import UNet
    torch.manual_seed(seed)
    return UNet(1, C, 8, norm_type="instance", act_type="lrelu").to(dev).eval()


@pytest.mark.parametrize("nets,tta", [(1, "d4"), (2, "flips")], ids=["unet-d4", "two-unets-flips"])
def test_real_network_against_fp64(dev, nets, tta):
    from smsut_amd import ops
    from smsut_amd.predict import Predictor
    models = [small_unet(21 + i, dev) for i in range(nets)]
    seen = []

    def recording(m):
        def f(x):
            out = m(x)
            seen.append(out)
            return out
        return f
    img = torch.from_numpy(np.random.default_rng(8).integers(0, 256, (4, 32, 32), dtype=np.uint8)).to(dev)
    tr = ops.tta_transforms(tta)
    pred, conf = Predictor([recording(m) for m in models], batch_size=4, tta=tta).predict_slices(img, confidence=True)
    assert len(seen) == nets * len(tr) == 8
    members = [z.permute(0, 2, 3, 1).cpu() for z in seen]       # the logits the predictor merged, [N, H, W, C]
    rpred, rconf, _, rgap = R.merge_ref(members, tr * nets)
    b = R.budget(C, 8)
    decided = rgap >= 4 * b
    left_out = float((~decided).double().mean())
    err = float((conf.cpu().double() - rconf).abs().max())
    print(f"{nets} U-Net(s) x {tta}: pixels left out = {left_out:.4%}, smallest gap = {float(rgap.min()):.3e}, "
          f"max |conf - ref| = {err:.3e}, B = {b:.3e}, classes predicted = {torch.unique(rpred).tolist()}")
    assert left_out <= 0.005
    assert torch.equal(pred.cpu().long()[decided], rpred[decided])
    assert err <= b
    for t, z in enumerate(seen[:len(tr)]):                      # member t really is the network on F_g of the slices
        assert torch.equal(z, models[0](R.fwd(loader_float(img), tr[t]).unsqueeze(1).contiguous()))


def test_cli_writes_the_files(dev, tmp_path, monkeypatch):
    from smsut_amd import config as cfg
    from smsut_amd import predict as P
    from smsut_amd.network.unet import UNet
    monkeypatch.setattr(cfg, "expr_root", str(tmp_path / "runs"))
    ckpt = tmp_path / "runs" / "UnetTrainer" / "000" / "ckpt"
    ckpt.mkdir(parents=True)
    torch.manual_seed(31)
    net = UNet(cfg.img_channels, cfg.n_label + 1, cfg.base_width, norm_type="instance", act_type="lrelu")
    torch.save({k: v.contiguous() for k, v in net.state_dict().items()}, ckpt / "last.ckpt")
    rng = np.random.default_rng(6)
    vol = (rng.standard_normal((3, 48, 40)) * 200.0).astype(np.float32)
    np.save(tmp_path / "scan.npy", vol)
    out = tmp_path / "out"
    P.main(["--trainer", "unet", "-i", "000", "--image", str(tmp_path / "scan.npy"), "--spacing", "5.0", "1.5", "1.5",
            "--modality", "ct", "--tta", "flips", "--confidence", "--out", str(out)])
    labels, proc, conf = (np.load(out / f) for f in ("labels.npy", "labels_processed.npy", "confidence.npy"))
    assert labels.shape == vol.shape and labels.dtype == np.uint8
    assert proc.shape == (3, 256, 256) and conf.shape == proc.shape and conf.dtype == np.float32
    assert 1.0 / (cfg.n_label + 1) - 1e-6 <= conf.min() and conf.max() <= 1.0 + 1e-6
    net.load_state_dict(torch.load(ckpt / "last.ckpt", map_location="cpu"))
    ref = P.predict_volume(P.Predictor(net.to(dev), tta="flips", classes=cfg.n_label + 1), vol, (5.0, 1.5, 1.5), "ct", confidence=True)
    assert np.array_equal(labels, ref.labels.cpu().numpy())
    assert np.array_equal(proc, ref.labels_processed.cpu().numpy())
