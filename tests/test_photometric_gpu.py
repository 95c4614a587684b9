"""The photometric augmentation on the device (csrc/photometric.hip: ``smsut_photo_hist`` + ``smsut_photo_apply``) against
Pillow's outputs (tests/golden/photometric_pil.npz) and the numpy restatement of its definition (tests/photometric_ref.py).

The bar is BIT EQUALITY, derived rather than measured: every step maps 8-bit levels to 8-bit levels, the histogram is integer
adds, and the blends are IEEE fp32 multiply and add in a fixed order without contraction -- there is no rounding freedom left."""
import random

import numpy as np
import pytest
import torch

import photometric_ref as R

pytestmark = pytest.mark.gpu


def _ga():
    import smsut_amd  # noqa: F401
    from smsut_amd.data_loader import gpu_augment as ga
    return ga


def unit(img8):
    """uint8 [N,H,W] -> fp32 [N,1,H,W] on the [0, 1] scale, on the device (IEEE quotient, computed on the host)."""
    return torch.from_numpy((np.asarray(img8, dtype=np.float32) / np.float32(255.0))[:, None]).cuda()


def levels(out):
    v = out.detach().cpu().numpy().astype(np.float64) * 255.0
    lv = np.rint(v)
    assert np.abs(v - lv).max() < 1e-3                       # the outputs sit on the 8-bit grid
    return lv.astype(np.uint8).reshape(out.shape[0], out.shape[-2], out.shape[-1])


def test_kernels_equal_pillow_on_every_fixture_pixel(golden):
    """Brightness alone, contrast alone, both orders, gamma alone, all three: zero mismatching pixels against Pillow.  The 27 cases
    of an image run as ONE batch of 27 slices with their own parameter rows; the gamma-alone cases run again without jitter (the
    single-launch path without a histogram)."""
    ga = _ga()
    g = golden("photometric_pil")
    args = [R.case_args(row) for row in g["params"]]
    seen = set()
    for name in g["names"]:
        img = g[f"img_{name}"]
        x = unit(np.repeat(img[None], len(args), 0))
        jit = [j if j is not None else (0, 1.0, 1.0) for (j, _) in args]
        out = ga.photometric(x, jit, [gm for (_, gm) in args])
        got = levels(out)
        for k, kind in enumerate(g["kinds"]):
            bad = int((got[k] != g[f"out_{name}"][k]).sum())
            assert bad == 0, (name, k, kind, g["params"][k], bad)
            seen.add(str(kind))
        gk = [k for k, (j, _) in enumerate(args) if j is None]
        out = ga.photometric(x[gk], None, [args[k][1] for k in gk])
        assert np.array_equal(levels(out), g[f"out_{name}"][gk]), name
    assert seen == {"brightness", "contrast", "both", "gamma", "all"}


def _hist_ref(lv):
    return np.stack([np.bincount(s.ravel(), minlength=256) for s in lv])


@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 33, 47), (2, 256, 256), (2, 400, 700)])
def test_histogram_equals_bincount(shape):
    """(1, 5, 7): less than one workgroup's chunk, H*W no multiple of 4.  (3, 33, 47): an odd H*W, so every slice starts at another
    offset to the 16-byte grid (scalar head and tail), different content per slice.  (2, 256, 256): 16 workgroups per slice.
    (2, 400, 700): more chunks than workgroups per slice (the cap of 16), so workgroups loop.  Slice 0 is full-range noise, the
    others are >= 90 % black with a few levels (the wave-level vote path)."""
    ga = _ga()
    n, h, w = shape
    rs = np.random.RandomState(h)
    lv = rs.randint(0, 256, shape).astype(np.uint8)
    for k in range(1, n):
        lv[k][rs.rand(h, w) < 0.92] = 0
        lv[k][rs.rand(h, w) < 0.02] = 255
    hist = ga.level_histogram(unit(lv))
    assert hist.dtype == torch.int32 and tuple(hist.shape) == (n, 256)
    assert np.array_equal(hist.cpu().numpy(), _hist_ref(lv))
    part = ga.level_histogram(unit(lv), _partials=True)
    assert part.shape[1] == max(1, min(16, -(-h * w // 4096)))


@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 33, 47), (2, 256, 256), (2, 400, 700)])
def test_apply_equals_restatement_on_every_path(shape):
    """The same shapes through the whole pass (mixed orders, gamma drawn and not) against the restatement.  (2, 400, 700) is more
    than 64 workgroups x 4 prefetched float4 per thread cover, so the apply kernel's streaming loop runs too."""
    ga = _ga()
    n, h, w = shape
    rs = np.random.RandomState(w)
    lv = rs.randint(0, 256, shape).astype(np.uint8)
    for k in range(1, n):
        lv[k][rs.rand(h, w) < 0.92] = 0
    jit = [(k % 2, 0.65 + 0.3 * k, 1.35 - 0.3 * k) for k in range(n)]
    gam = [None if k % 2 else 0.8 + 0.3 * k for k in range(n)]
    got = levels(ga.photometric(unit(lv), jit, gam))
    for k in range(n):
        assert np.array_equal(got[k], R.apply(lv[k], jit[k], gam[k])), k


def test_histogram_of_the_sparse_fixture_image_and_of_an_unaligned_view(golden):
    ga = _ga()
    g = golden("photometric_pil")
    img = g["img_sparse"]
    assert (img == 0).mean() >= 0.9
    hist = ga.level_histogram(unit(img[None]))
    assert np.array_equal(hist.cpu().numpy(), _hist_ref(img[None]))
    # a contiguous view whose base is not 16-byte aligned: the all-scalar path
    lv = np.random.RandomState(1).randint(0, 256, (3, 33, 47)).astype(np.uint8)
    x = unit(lv)[1:]
    assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    assert np.array_equal(ga.level_histogram(x).cpu().numpy(), _hist_ref(lv[1:]))
    jit, gam = [(0, 1.3, 0.7), (1, 0.8, 1.25)], [0.9, None]
    out = ga.photometric(x, jit, gam)
    assert np.array_equal(levels(out), np.stack([R.apply(lv[1 + k], jit[k], gam[k]) for k in range(2)]))


def test_quantisation():
    """(l + d) / 255 for all 256 levels and d in {-0.49, -0.2, 0, 0.2, 0.49} is level l (floor(x * 255 + 0.5): no input is closer
    than 0.01 level to a tie, where fp32 rounding of x * 255 -- at most 255 * 2^-24 * 2 = 3e-5 level -- cannot reach); below 0 is 0,
    above 1 is 255."""
    ga = _ga()
    ds = (-0.49, -0.2, 0.0, 0.2, 0.49)
    lv = np.arange(256, dtype=np.float64)
    x = np.stack([((lv + d) / 255.0).reshape(16, 16) for d in ds]).astype(np.float32)
    xt = torch.from_numpy(x[:, None]).cuda()
    out = ga.photometric(xt)
    want = (np.arange(256, dtype=np.float32) / np.float32(255.0)).reshape(16, 16)
    assert all(np.array_equal(out[k, 0].cpu().numpy(), want) for k in range(len(ds)))
    assert np.array_equal(ga.level_histogram(xt).cpu().numpy(), np.ones((len(ds), 256), np.int32))
    far = torch.tensor([[-0.3, -1e-2, -100.0, 0.0], [1.0, 1.0 + 1e-2, 1.7, 300.0]], device="cuda").reshape(2, 1, 1, 4)
    got = ga.photometric(far)
    assert np.array_equal(levels(got), np.array([[[0, 0, 0, 0]], [[255, 255, 255, 255]]]))
    h = ga.level_histogram(far).cpu().numpy()
    assert h[0, 0] == 4 and h[1, 255] == 4 and h.sum() == 8


def test_identity_and_normalize_parity():
    """b = c = 1, no gamma, an image holding all 256 levels, fed as the loader feeds it (uint8 -> float().div_(255.0)):
    ``normalize=False`` gives exactly level / 255; ``normalize=True`` is bit-identical to the loader's present chain."""
    ga = _ga()
    rs = np.random.RandomState(2)
    lv = np.stack([rs.permutation(256).reshape(16, 16), rs.permutation(256).reshape(16, 16)]).astype(np.uint8)
    img8 = torch.from_numpy(lv).cuda()
    x = img8.float().div_(255.0).unsqueeze(1)
    jit = [(0, 1.0, 1.0), (1, 1.0, 1.0)]
    out = ga.photometric(x, jit, [None, None])
    assert np.array_equal(out[:, 0].cpu().numpy(), lv.astype(np.float32) / np.float32(255.0))
    outn = ga.photometric(x, jit, [None, None], normalize=True)
    assert torch.equal(outn, img8.float().div_(255.0).unsqueeze(1).sub_(0.5).div_(0.5))
    aug = ga.GpuPhotometricAugment(dict(colorJitter=True))
    assert torch.equal(aug(x, params=(jit, None), normalize=True), outn)
    # gamma 1.0 drawn is the identity too (its table is)
    assert torch.equal(ga.photometric(x, None, [1.0, 1.0], normalize=True), outn)


def test_batch_independence():
    """A slice alone with its own parameters is bit-identical to its rows in a batch of 4 with mixed parameters (both orders, gamma
    drawn and not) -- and both equal the restatement.  33 x 47: in the batch every slice sits at another 16-byte offset."""
    ga = _ga()
    rs = np.random.RandomState(3)
    lv = rs.randint(0, 256, (4, 33, 47)).astype(np.uint8)
    lv[2][rs.rand(33, 47) < 0.9] = 0
    x = unit(lv)
    jit = [(0, 0.7, 1.3), (1, 1.35, 0.65), (1, 0.9, 1.1), (0, 1.2, 1.4)]
    gam = [1.3, None, 0.8, None]
    for norm in (False, True):
        out = ga.photometric(x, jit, gam, normalize=norm)
        for k in range(4):
            one = ga.photometric(x[k:k + 1].clone(), [jit[k]], [gam[k]], normalize=norm)
            assert torch.equal(one[0], out[k]), (k, norm)
    got = levels(ga.photometric(x, jit, gam))
    for k in range(4):
        assert np.array_equal(got[k], R.apply(lv[k], jit[k], gam[k])), k
    assert not np.array_equal(got, lv)


class _Stub:
    """What InTurnLoader reads of a dataset: uint8 images / labels in RAM, modality, names."""

    def __init__(self, n=6, size=32, seed=4):
        rs = np.random.RandomState(seed)
        img = rs.randint(0, 256, (n, size, size)).astype(np.uint8)
        img[:, :6, :] = 0
        self.images = torch.from_numpy(img)
        self.labels = torch.from_numpy(rs.randint(0, 5, (n, size, size)).astype(np.uint8))
        self.modality = [0, 0, 0, 0, 1, 1]
        self.names = [f"m_{i:03d}_000" for i in range(n)]
        self.modal_sample_ids = [[0, 1, 2, 3], [4, 5]]


def _norm_chain(img8):
    return img8.cuda().float().div_(255.0).unsqueeze(1).sub_(0.5).div_(0.5)          # the loader's chain without augmentation


def test_loader_applies_the_drawn_parameters_exactly():
    ga = _ga()
    from smsut_amd import config as cfg
    from smsut_amd.data_loader import inTurnLoader as inlod
    ds = _Stub()
    sampler = inlod.InTurnTestBatchSampler(ds.modal_sample_ids, 2)
    flags = dict(cfg.data_aug, rotate=False, elasticDeform=False, resizeCrop=False, colorJitter=True, gammaCorrect=True)
    photo = ga.GpuPhotometricAugment(flags)
    random.seed(11)
    batches = list(inlod.InTurnLoader(ds, sampler, "cuda", None, photo))
    assert [len(b[3]) for b in batches] == [2, 2, 2]
    random.seed(11)
    changed = 0
    for (img, msk, mdl, names), ids in zip(batches, sampler):
        jit, gam = photo.draw(len(ids))
        want8 = np.stack([R.apply(ds.images[i].numpy(), jit[k], gam[k]) for k, i in enumerate(ids)])
        assert torch.equal(img, _norm_chain(torch.from_numpy(want8))), ids
        assert torch.equal(msk.cpu(), ds.labels[ids].to(torch.int64)) and names == [ds.names[i] for i in ids]
        changed += int(not np.array_equal(want8, ds.images[ids].numpy()))
    assert changed == 3
    # photometric flags off: the loader's output is what its chain yielded before
    off = ga.GpuPhotometricAugment(dict(flags, colorJitter=False, gammaCorrect=False))
    for (img, msk, mdl, names), ids in zip(inlod.InTurnLoader(ds, sampler, "cuda", None, off), sampler):
        assert torch.equal(img, _norm_chain(ds.images[ids]))
        assert torch.equal(msk.cpu(), ds.labels[ids].to(torch.int64))


def test_loader_with_geometric_and_photometric_augmentation():
    ga = _ga()
    from smsut_amd import config as cfg
    from smsut_amd.data_loader import inTurnLoader as inlod
    ds = _Stub()
    sampler = inlod.InTurnTestBatchSampler(ds.modal_sample_ids, 2)
    flags = dict(cfg.data_aug, resizeCrop_size=24, colorJitter=True, gammaCorrect=True)
    joint, photo = ga.GpuJointAugment(flags, 24), ga.GpuPhotometricAugment(flags)
    random.seed(12)
    both = list(inlod.InTurnLoader(ds, sampler, "cuda", joint, photo))
    grid = ga.level_table("cuda", True)
    # the same joint draws without the photometric pass: its draws are made by hand between the batches to keep the stream aligned
    random.seed(12)
    geo = []
    for b in inlod.InTurnLoader(ds, sampler, "cuda", joint, None):
        geo.append(b)
        photo.draw(len(b[3]))
    differs = 0
    for (img, msk, _, _), (gimg, gmsk, _, _) in zip(both, geo):
        assert tuple(img.shape) == (2, 1, 24, 24) and tuple(msk.shape) == (2, 24, 24) and msk.dtype == torch.int64
        assert float(img.min()) >= -1.0 and float(img.max()) <= 1.0
        assert bool(torch.isin(img, grid).all())                                     # every value lies on the 256-level grid
        assert torch.equal(msk, gmsk)                                                # labels are untouched by the photometric pass
        differs += int(not torch.equal(img, gimg))
    assert differs == 3
