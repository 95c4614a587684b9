"""CPU checks of the photometric augmentation (ColorJitter + RandomGammaCorrection, reference data_loader/baseLoader.py:102-109):
the numpy restatement the GPU tests use as their reference (tests/photometric_ref.py) reproduces every pixel Pillow produced
(tests/golden/photometric_pil.npz), the host gamma-table builder equals the fixture's tables, and the parameter draws follow the
reference's distributions.  No kernel runs here."""
import random

import numpy as np
import pytest
import torch

import photometric_ref as R


def test_restatement_equals_pillow_on_every_pixel(golden):
    g = golden("photometric_pil")
    assert np.array_equal(g["params"], np.array([c[1:] for c in R.cases()], dtype=np.float64), equal_nan=True)   # the shared case list
    assert g["kinds"].tolist() == [c[0] for c in R.cases()]
    kinds = set(g["kinds"].tolist())
    assert kinds == {"brightness", "contrast", "both", "gamma", "all"}
    imgs = R.images()
    assert sorted(imgs) == g["names"].tolist()
    for name in g["names"]:
        img = g[f"img_{name}"]
        assert np.array_equal(img, imgs[name]) and img.dtype == np.uint8
        changed = 0
        for k, row in enumerate(g["params"]):
            jit, gam = R.case_args(row)
            out = R.apply(img, jit, gam)
            assert np.array_equal(out, g[f"out_{name}"][k]), (name, k, g["kinds"][k], row)
            changed += int(not np.array_equal(out, img))
        assert changed >= (10 if name != "const" else 5), (name, changed)       # the cases really do something
    assert (g["img_sparse"] == 0).mean() >= 0.9 and g["img_low"].max() <= 63 and len(np.unique(g["img_const"])) == 1
    assert len(np.unique(g["img_rand"])) > 200


def test_both_orders_differ_somewhere(golden):
    """The order of brightness and contrast is observable (truncation and the mean of the intermediate image): the fixture holds
    pairs that differ, so a chain that ignored the order flag would fail the pixel test."""
    g = golden("photometric_pil")
    p = g["params"]
    both = [k for k, kind in enumerate(g["kinds"]) if kind == "both"]
    o0 = {(p[k][1], p[k][2]): k for k in both if p[k][0] == 0}
    o1 = {(p[k][1], p[k][2]): k for k in both if p[k][0] == 1}
    assert set(o0) == set(o1) and len(o0) == len(R.PAIRS)
    assert any(not np.array_equal(g["out_rand"][o0[bc]], g["out_rand"][o1[bc]]) for bc in o0)


def test_gamma_table_builder_equals_the_fixture_tables(golden):
    import smsut_amd  # noqa: F401
    from smsut_amd.data_loader import gpu_augment as ga
    g = golden("photometric_pil")
    for gamma, tab in zip(g["gammas"], g["gamma_tables"]):
        t = ga.gamma_table(float(gamma))
        assert t.dtype == np.uint8 and t.shape == (256,)
        assert np.array_equal(t, tab) and np.array_equal(R.gamma_table(gamma), tab)
    assert np.array_equal(ga.gamma_table(1.0), np.arange(256))


def test_quantise_restatement():
    lv = np.arange(256)
    for d in (-0.49, -0.2, 0.0, 0.2, 0.49):
        assert np.array_equal(R.quantise((lv + d) / 255.0), lv)
    assert np.array_equal(R.quantise([-0.3, -1e-3, 1.0 + 1e-3, 7.0]), [0, 0, 255, 255])


def test_draw_ranges_orders_coin_and_seed():
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    from smsut_amd.data_loader import gpu_augment as ga
    aug = ga.GpuPhotometricAugment(dict(cfg.data_aug, colorJitter=True, gammaCorrect=True))
    assert aug.enabled and (aug.brightness, aug.contrast) == (0.4, 0.4)
    random.seed(3)
    jit, gam = aug.draw(4000)
    assert len(jit) == len(gam) == 4000
    o, b, c = (np.array(v) for v in zip(*jit))
    assert set(o.tolist()) == {0, 1} and 0.45 < o.mean() < 0.55                          # a fair coin: 4000 draws, sigma 0.008
    for f in (b, c):
        assert 0.6 <= f.min() < 0.62 and 1.38 < f.max() <= 1.4 and abs(f.mean() - 1.0) < 0.02
    drawn = np.array([v for v in gam if v is not None])
    assert 0.45 < len(drawn) / 4000 < 0.55
    lo, hi = cfg.data_aug["gammaCorrect_gammas"]
    assert lo <= drawn.min() < lo + 0.02 and hi - 0.02 < drawn.max() <= hi
    random.seed(3)
    jit2, gam2 = aug.draw(4000)
    assert jit2 == jit and gam2 == gam                                                   # a fixed seed gives fixed parameters
    random.seed(4)
    assert aug.draw(8) != (jit[:8], gam[:8])
    # one flag alone draws only its own parameters
    random.seed(5)
    j, gm = ga.GpuPhotometricAugment(dict(colorJitter=True)).draw(3)
    assert gm is None and len(j) == 3
    j, gm = ga.GpuPhotometricAugment(dict(gammaCorrect=True, gammaCorrect_gammas=(0.7, 1.5))).draw(3)
    assert j is None and len(gm) == 3
    # subclass attributes change the strengths
    class Weak(ga.GpuPhotometricAugment):
        brightness = 0.1
    jw, _ = Weak(dict(colorJitter=True)).draw(200)
    assert all(0.9 <= t[1] <= 1.1 for t in jw)


def test_disabled_when_both_flags_are_off_and_loader_drops_it():
    import smsut_amd  # noqa: F401
    from smsut_amd import config as cfg
    from smsut_amd.data_loader import gpu_augment as ga, inTurnLoader as inlod
    assert cfg.data_aug["colorJitter"] is False and cfg.data_aug["gammaCorrect"] is False
    off = ga.GpuPhotometricAugment(cfg.data_aug)
    assert not off.enabled and not ga.GpuPhotometricAugment(None).enabled
    state = random.getstate()
    assert off.draw(5) == (None, None) and random.getstate() == state                    # and consumes no random numbers
    assert ga.GpuPhotometricAugment(dict(cfg.data_aug, colorJitter=True)).enabled
    assert ga.GpuPhotometricAugment(dict(cfg.data_aug, gammaCorrect=True)).enabled
    ld = inlod.InTurnLoader(None, [], "cpu", None, off)
    assert ld.photometric is None                                                        # the loader keeps its present chain
    on = ga.GpuPhotometricAugment(dict(cfg.data_aug, gammaCorrect=True))
    assert inlod.InTurnLoader(None, [], "cpu", None, on).photometric is on


def test_cpu_tensors_are_refused():
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    from smsut_amd.data_loader import gpu_augment as ga
    x = torch.rand(2, 1, 8, 8)
    with pytest.raises(_hip.SmsutHipError):
        ga.photometric(x, [(0, 1.1, 0.9)] * 2, [None, 1.2])
    with pytest.raises(_hip.SmsutHipError):
        ga.GpuPhotometricAugment(dict(colorJitter=True))(x)
    with pytest.raises(_hip.SmsutHipError):
        ga.level_histogram(x)


def test_get_loader_builds_the_pass_when_a_flag_is_set(tmp_path):
    """``get_loader`` over a small PNG dataset: train / val loaders carry the photometric pass exactly when ``colorJitter`` or
    ``gammaCorrect`` is set; the test phase never does.  With it set, a CPU loader refuses loudly instead of dropping the pass."""
    yaml = pytest.importorskip("yaml")
    Image = pytest.importorskip("PIL.Image")
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip, config as cfg
    from smsut_amd.data_loader import gpu_augment as ga, inTurnLoader as inlod
    rs = np.random.RandomState(0)
    split = {}
    for m in ("ct", "t1in", "t1out", "t2"):
        split[m] = {"train": [["001"]], "val": [["002"]], "test": ["003"]}
        for pid in ("001", "002", "003"):
            for sub, hi in (("images", 255), ("labels", 5)):
                (tmp_path / m / pid / sub).mkdir(parents=True)
                for z in range(4):
                    Image.fromarray(rs.randint(0, hi, (16, 16)).astype(np.uint8)).save(tmp_path / m / pid / sub / f"{m}_{pid}_{z:03d}.png")
    with open(tmp_path / "split.yaml", "w") as f:
        yaml.dump(split, f)
    random.seed(2)

    def mk(phase, aug):
        return inlod.get_loader(str(tmp_path), phase, 0, 2, data_aug=aug, device="cpu", split_yaml="split.yaml")
    assert mk("train", cfg.data_aug).photometric is None and mk("train", None).photometric is None
    for flag in ("colorJitter", "gammaCorrect"):
        on = dict(cfg.data_aug, **{flag: True})
        for phase in ("train", "val"):
            ld = mk(phase, on)
            assert isinstance(ld.photometric, ga.GpuPhotometricAugment) and ld.photometric.enabled
        assert mk("test", None).photometric is None
    plain = dict(cfg.data_aug, rotate=False, elasticDeform=False, resizeCrop=False)
    img = next(iter(inlod.InTurnLoader(mk("train", plain).ds, [[0, 1]], "cpu", None, ga.GpuPhotometricAugment(plain))))[0]
    assert tuple(img.shape) == (2, 1, 16, 16)                                            # flags off: the present chain, on any device
    with pytest.raises(_hip.SmsutHipError):
        next(iter(inlod.InTurnLoader(mk("train", plain).ds, [[0, 1]], "cpu", None, ga.GpuPhotometricAugment(dict(plain, colorJitter=True)))))
