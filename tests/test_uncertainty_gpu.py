"""``ops.tta_uncertainty`` (csrc/uncertainty.hip), ``Predictor.predict_uncertain`` and ``predict_volume(uncertainty=True)`` on the
device, against tests/uncertainty_ref.py.

Cases (uncertainty_ref.CASES): 20 x 20 is a partial tile of both tile sizes; 37 x 50 is non-square with 2 x 2 tiles of 32 and rows
that start off a 16-byte boundary; 40 x 40 puts the quarter turns on 2 x 2 tiles; (7, 3) is K < C; (4, 4) an even C (padded pixel
stride in LDS); (12, 12) the runtime class loop on staged 16 x 16 tiles; (33, 32) rows read in place with K at its limit; T = 16
fills both words of the packed member labels; one pixel with one member; one class.  The members are drawn as uamt_ref.case draws
(H spreads over [0, ln K], the members partly agree) and put on their transformed grids.

Bounds, absolute, on every pixel: |entropy - H64| <= B_H = uamt_ref.entropy_bound(K, T); |mutual_info - MI64| <= B_MI (derived in
tests/uncertainty_ref.py).  The integers are exact: votes and counts are compared with host counts built from
``ops.argmax_channels`` of every member, the kernel's own ``pred`` and rint(entropy * 2^20) of the kernel's own entropy, so no pixel
is excluded for a near-tie; ``pred`` itself must equal the fp64 reference's wherever the reference's top-two gap is at least
4 x tta_ref.budget(K, T), which may leave out at most 0.5 % of a case's pixels (asserted; the seed is checked on the CPU in
tests/test_uncertainty_cpu.py)."""
import numpy as np
import pytest
import torch

import tta_ref as R
import uncertainty_ref as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import smsut_amd  # noqa: F401
    return torch.device("cuda")


@pytest.fixture(scope="module")
def cases():
    """Members and fp64 references of every case, computed once"""
    members = U.draw_cases()
    return [(zs, U.reference(zs, tr, k)) for zs, (t, n, h, w, c, k, tr, off) in zip(members, U.CASES)]


def to_member(z, dev, offset=False):
    """NHWC array [N, H, W, C] -> the logical NCHW tensor over that memory (what a network here returns); ``offset``: a view that
    starts one float into its allocation."""
    t = torch.from_numpy(np.ascontiguousarray(z))
    if offset:
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=dev)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
    else:
        v = t.to(dev)
    return v.permute(0, 3, 1, 2)


def new_counts(k, t, dev):
    return torch.zeros(k, 2 * t + 4, dtype=torch.int64, device=dev)


def device_labels(members, tr, k):
    """int64 [T, N, H, W] on the host: ``ops.argmax_channels`` of every member's K leading channels, put back with ``tta_ref.inv``"""
    from smsut_amd import ops
    return np.stack([R.inv(ops.argmax_channels(m[:, :k]), g).cpu().numpy() for m, g in zip(members, tr)])


def run(idx, cases, dev, **kw):
    from smsut_amd import ops
    t, n, h, w, c, k, tr, off = U.CASES[idx]
    members = [to_member(z, dev, off) for z in cases[idx][0]]
    counts = new_counts(k, t, dev)
    return members, counts, ops.tta_uncertainty(members, tr, classes=k, counts=counts, **kw)


# ---------------------------------------------------------------------------------------------- 1. the merge's prediction
@pytest.mark.parametrize("idx", range(len(U.CASES)), ids=U.IDS)
def test_same_prediction_as_the_merge(dev, cases, idx):
    from smsut_amd import ops
    t, n, h, w, c, k, tr, off = U.CASES[idx]
    before = ops.layout_copies()
    members, counts, u = run(idx, cases, dev)
    assert ops.layout_copies() == before                        # NHWC members are read in place
    pred, conf, _ = ops.tta_merge(members, tr, classes=k, want_conf=True)
    assert u.pred.dtype == torch.uint8 and u.votes.dtype == torch.uint8 and u.entropy.dtype == u.mutual_info.dtype == torch.float32
    assert all(x.shape == (n, h, w) for x in u)
    assert torch.equal(u.pred, pred) and torch.equal(u.conf, conf)
    lean = ops.tta_uncertainty(members, tr, classes=k, want_maps=False)        # neither maps nor counts: the merge alone
    assert lean.entropy is None and lean.mutual_info is None and lean.votes is None
    assert torch.equal(lean.pred, pred) and torch.equal(lean.conf, conf)


# ---------------------------------------------------------------------------------------------- 2. maps against fp64
@pytest.mark.parametrize("idx", range(len(U.CASES)), ids=U.IDS)
def test_maps_against_fp64(dev, cases, idx):
    t, n, h, w, c, k, tr, off = U.CASES[idx]
    _, (rpred, rconf, rh, reh, rmi, rgap) = cases[idx]
    _, _, u = run(idx, cases, dev)
    eh = float((u.entropy.cpu().double() - rh).abs().max())
    emi = float((u.mutual_info.cpu().double() - rmi).abs().max())
    print(f"tta_uncertainty {U.IDS[idx]}: max |H - ref| = {eh:.3e} (B_H = {U.bound_h(k, t):.3e}), max |MI - ref| = {emi:.3e} "
          f"(B_MI = {U.bound_mi(k, t):.3e}); H in [{float(rh.min()):.4f}, {float(rh.max()):.4f}], MI up to {float(rmi.max()):.4f}")
    assert eh <= U.bound_h(k, t)
    assert emi <= U.bound_mi(k, t)
    assert float(u.mutual_info.min()) >= 0.0
    if t == 1:                                                  # one member: H and EH are the same bits
        assert torch.all(u.mutual_info == 0) and torch.all(u.votes == 1)
    if k == 1:
        # every entropy is -logf(1 + 1e-6f): one value, and that value is the fp32 neighbour of the exact logarithm of the fp32
        # sum (the device library documents logf within 1 ulp)
        x = np.float32(1) + np.float32(1e-6)
        want = np.float32(-np.log(np.float64(x)))
        got = u.entropy.cpu().numpy()
        print(f"one class: entropy {got.flat[0]!r}, -log(fl(1 + 1e-6f)) = {want!r}")
        assert np.all(got == got.flat[0]) and abs(np.float64(got.flat[0]) - np.float64(want)) <= np.spacing(np.abs(want))
        assert torch.all(u.votes == t) and torch.all(u.pred == 0)


# ---------------------------------------------------------------------------------------------- 3. integers, exact
@pytest.mark.parametrize("idx", range(len(U.CASES)), ids=U.IDS)
def test_integers_exact(dev, cases, idx):
    t, n, h, w, c, k, tr, off = U.CASES[idx]
    zs, (rpred, rconf, rh, reh, rmi, rgap) = cases[idx]
    members, counts, u = run(idx, cases, dev)
    labels = device_labels(members, tr, k)
    assert np.array_equal(labels, U.member_labels(zs, tr, k))                  # (argmax_channels is exact: the host agrees)
    pred = u.pred.cpu().numpy().astype(np.int64)
    assert np.array_equal(u.votes.cpu().numpy(), U.votes_of(labels, pred))
    want = U.counts_of(pred, labels, u.entropy.cpu().numpy(), k)
    got = counts.cpu().numpy()
    assert got.shape == want.shape == (k, 2 * t + 4)
    assert np.array_equal(got, want), f"counts differ at (class, slot) {np.argwhere(got != want).tolist()[:8]}"
    assert got[:, U.V].sum() == n * h * w
    decided = rgap >= 4 * R.budget(k, t)
    left_out = float((~decided).double().mean())
    assert left_out <= 0.005
    assert torch.equal(u.pred.cpu().long()[decided], rpred[decided])


# ---------------------------------------------------------------------------------------------- 4. accumulation, reproducibility
def test_counts_accumulate(dev, cases):
    from smsut_amd import ops
    t, n, h, w, c, k, tr, off = U.CASES[0]
    a = [to_member(z, dev) for z in cases[0][0]]
    b = [to_member(z, dev) for z in U.draw(t, n, h, w, c, tr, np.random.RandomState(77))]
    ca, cb, both = (new_counts(k, t, dev) for _ in range(3))
    ops.tta_uncertainty(a, tr, counts=ca)
    ops.tta_uncertainty(b, tr, counts=cb)
    ops.tta_uncertainty(a, tr, counts=both)
    ops.tta_uncertainty(b, tr, counts=both, want_maps=False)    # (the counts do not depend on the maps being asked for)
    assert int(ca.sum()) > 0 and not torch.equal(ca, cb)
    assert torch.equal(both, ca + cb)


def test_three_slices_of_several_tiles(dev):
    from smsut_amd import ops
    t, n, h, w, c, tr = 4, 3, 37, 50, 5, U.FLIPS
    zs = U.draw(t, n, h, w, c, tr, np.random.RandomState(78))
    members = [to_member(z, dev) for z in zs]
    counts = new_counts(c, t, dev)
    u = ops.tta_uncertainty(members, tr, counts=counts)
    pred = u.pred.cpu().numpy().astype(np.int64)
    labels = U.member_labels(zs, tr, c)
    assert np.array_equal(counts.cpu().numpy(), U.counts_of(pred, labels, u.entropy.cpu().numpy(), c))
    assert np.array_equal(u.votes.cpu().numpy(), U.votes_of(labels, pred))
    assert int(counts[:, U.V].sum()) == n * h * w


def test_two_calls_are_bitwise_equal(dev, cases):
    _, ca, a = run(1, cases, dev)
    _, cb, b = run(1, cases, dev)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(ca, cb)


def test_no_slices_and_refusals(dev):
    from smsut_amd import ops
    z = lambda *s: torch.zeros(*s, device=dev).permute(0, 3, 1, 2)
    counts = new_counts(5, 1, dev)
    u = ops.tta_uncertainty([z(0, 4, 4, 5)], (0,), counts=counts)               # N == 0: empty tensors, no launch
    assert all(x.shape == (0, 4, 4) for x in u) and int(counts.sum()) == 0
    with pytest.raises(ValueError):                             # [classes, 2 T + 4] for T = 2 is [5, 8]
        ops.tta_uncertainty([z(1, 4, 4, 5)] * 2, (0, 4), counts=counts)
    with pytest.raises(ValueError):                             # not contiguous
        ops.tta_uncertainty([z(1, 4, 4, 5)], (0,), counts=torch.zeros(6, 5, dtype=torch.int64, device=dev).t())
    with pytest.raises(ValueError):                             # rows are the classes asked for
        ops.tta_uncertainty([z(1, 4, 4, 5)], (0,), classes=3, counts=counts)
    with pytest.raises(TypeError):                              # on the members' device
        ops.tta_uncertainty([z(1, 4, 4, 5)], (0,), counts=torch.zeros(5, 6, dtype=torch.int64))
    with pytest.raises(ValueError):                             # a quarter turn of a non-square slice
        ops.tta_uncertainty([z(1, 37, 50, 5)], (1,))
    with pytest.raises(ValueError):                             # K > C
        ops.tta_uncertainty([z(1, 4, 4, 5)], (0,), classes=6)
    assert int(counts.sum()) == 0


# ---------------------------------------------------------------------------------------------- 5. planted disagreement
def test_planted_disagreement(dev):
    """Member t carries 8 onehot(F_g(L)) + 0.1 noise for a label map L with no symmetry; then member 3 (a quarter turn) carries
    another label inside a rectangle that straddles the border between the 32 x 32 tiles.  A wrong inverse transform of the member
    labels moves the rectangle, or breaks the unanimity."""
    from smsut_amd import ops
    from smsut_amd.misc.utils import structure_agreement
    tr, n, s, c, odd = U.D4, 1, 40, 5, 3
    t = len(tr)
    rng = np.random.default_rng(11)
    lab = torch.from_numpy(rng.integers(0, c, (n, s, s)))
    lab2 = lab.clone()
    rect = (slice(None), slice(28, 36), slice(30, 37))
    lab2[rect] = (lab[rect] + 1) % c
    noise = [0.1 * torch.from_numpy(rng.standard_normal((n, s, s, c)).astype(np.float32)) for _ in tr]

    def members_of(label_of_member):
        return [to_member((8.0 * torch.nn.functional.one_hot(R.fwd(label_of_member(i), g), c).float() + noise[i]).numpy(), dev)
                for i, g in enumerate(tr)]

    counts = new_counts(c, t, dev)
    u = ops.tta_uncertainty(members_of(lambda i: lab), tr, counts=counts)
    cn = counts.cpu().numpy()
    assert torch.equal(u.pred.cpu().long(), lab) and torch.all(u.votes == t)
    assert np.array_equal(cn[:, U.ALL], cn[:, U.V]) and np.array_equal(cn[:, U.ANY], cn[:, U.V]) and cn[:, U.V].min() > 0
    assert np.array_equal(cn[:, U.FIXED:], np.repeat(cn[:, U.V:U.V + 1], 2 * t, axis=1))
    assert np.all(structure_agreement(counts, t).dice_agreement == 1.0)
    assert float(u.mutual_info.max()) < 1e-3

    counts = new_counts(c, t, dev)
    u = ops.tta_uncertainty(members_of(lambda i: lab2 if i == odd else lab), tr, counts=counts)
    cn = counts.cpu().numpy()
    inside = torch.zeros(n, s, s, dtype=torch.bool)
    inside[rect] = True
    assert torch.equal(u.pred.cpu().long(), lab)
    assert torch.equal(u.votes.cpu().long(), torch.where(inside, t - 1, t))
    labels = np.stack([(lab2 if i == odd else lab).numpy() for i in range(t)])
    assert np.array_equal(cn, U.counts_of(lab.numpy(), labels, u.entropy.cpu().numpy(), c))
    for k in set(lab[rect].flatten().tolist()) | set(lab2[rect].flatten().tolist()):
        assert cn[k, U.ANY] > cn[k, U.ALL]
    for k in set(lab[rect].flatten().tolist()):
        assert cn[k, U.FIXED + t + odd] < cn[k, U.V]            # that member's overlap with the consensus
        assert all(cn[k, U.FIXED + t + i] == cn[k, U.V] for i in range(t) if i != odd)
    assert float(u.mutual_info.cpu()[inside].min()) > float(u.mutual_info.cpu()[~inside].max())


# ---------------------------------------------------------------------------------------------- 6. a NaN logit
def test_one_nan_logit(dev, cases):
    from smsut_amd import ops
    t, n, h, w, c, k, tr, off = U.CASES[1]
    zs = [z.copy() for z in cases[1][0]]
    zs[2][0, 5, 7, 2] = np.nan
    members = [to_member(z, dev, off) for z in zs]
    counts = new_counts(k, t, dev)
    u = ops.tta_uncertainty(members, tr, counts=counts)
    pred, conf, _ = ops.tta_merge(members, tr, want_conf=True)
    assert torch.equal(u.pred, pred) and torch.equal(u.conf.view(torch.int32), conf.view(torch.int32))
    ent = u.entropy.cpu().numpy()
    hit = R.inv(torch.from_numpy(np.isnan(zs[2]).any(-1)), tr[2]).numpy()      # the output pixel that member's NaN lands on
    assert hit.sum() == 1 and np.array_equal(np.isnan(ent), hit)
    labels = device_labels(members, tr, k)
    assert labels[2][hit] == 2                                  # a NaN wins: that member's own label is the NaN's channel
    p = u.pred.cpu().numpy().astype(np.int64)
    assert p[hit] == 0                                          # (its softmax is NaN in every class, so is the mean: the first one)
    got = counts.cpu().numpy()
    assert np.array_equal(got, U.counts_of(p, labels, ent, k))                  # HSUM skips the pixel
    assert got[:, U.HSUM].sum() == np.rint(ent[~hit].astype(np.float64) * U.SCALE).astype(np.int64).sum()
    assert got[:, U.V].sum() == n * h * w                       # the other counters include it
    assert got[:, U.FIXED:U.FIXED + t].sum(0).tolist() == [n * h * w] * t
    assert np.array_equal(u.votes.cpu().numpy(), U.votes_of(labels, p))


# ---------------------------------------------------------------------------------------------- 7. the predictor
def small_unet(seed, dev, c=5):
    from smsut_amd.network.unet import UNet
    torch.manual_seed(seed)
    return UNet(1, c, 8, norm_type="instance", act_type="lrelu").to(dev).eval()


def test_predictor_uncertain(dev):
    from smsut_amd import ops
    from smsut_amd.predict import Predictor
    net, seen = small_unet(41, dev), []

    def recording(x):
        out = net(x)
        seen.append(out)
        return out
    img = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (5, 32, 32), dtype=np.uint8)).to(dev)
    tr = ops.tta_transforms("flips")
    u = Predictor(recording, batch_size=2, tta="flips").predict_uncertain(img)
    pred, conf = Predictor(net, batch_size=2, tta="flips").predict_slices(img, confidence=True)
    assert torch.equal(u.pred, pred) and torch.equal(u.conf, conf)
    assert len(seen) == 3 * len(tr) and all(z.shape[0] == 2 for z in seen)     # three groups of two, the last one padded
    total = new_counts(5, len(tr), dev)
    for g, count in enumerate((2, 2, 1)):
        outs = [z[:count] for z in seen[g * len(tr):(g + 1) * len(tr)]]
        part = ops.tta_uncertainty(outs, tr, counts=total)
        sl = slice(2 * g, 2 * g + count)
        assert torch.equal(part.entropy, u.entropy[sl]) and torch.equal(part.mutual_info, u.mutual_info[sl])
        assert torch.equal(part.votes, u.votes[sl])
    assert u.counts.shape == (5, 2 * len(tr) + 4) and torch.equal(u.counts, total)
    assert int(u.counts[:, U.V].sum()) == 5 * 32 * 32           # the padding counted nowhere
    assert torch.equal(u.counts[:, U.V].cpu(), torch.bincount(pred.flatten().long().cpu(), minlength=5))
    one = Predictor(net, batch_size=5, tta="none").predict_uncertain(img)      # one member still goes through the op
    assert torch.all(one.votes == 1) and torch.all(one.mutual_info == 0) and int(one.counts[:, U.V].sum()) == 5 * 32 * 32


def test_predict_volume_uncertainty(dev):
    from smsut_amd.misc.utils import StructureAgreement
    from smsut_amd.predict import Predictor, PredictResult, UncertainResult, predict_volume
    vol = (np.random.default_rng(4).standard_normal((12, 40, 44)) * 300.0).astype(np.float32)
    spacing = (5.0, 1.25, 1.25)                                 # -> a 12 x 33 x 36 grid, cropped to 32 x 32 in plane
    p = Predictor(small_unet(42, dev), batch_size=5, tta="flips")
    plain = predict_volume(p, vol, spacing, "ct", crop_size=32, confidence=True)
    assert type(plain) is PredictResult and len(plain) == 4
    r = predict_volume(p, vol, spacing, "ct", crop_size=32, confidence=True, uncertainty=True)
    assert type(r) is UncertainResult and r[:4][3] == plain.plan
    for a, b in zip(r[:3], plain[:3]):
        assert torch.equal(a, b)
    assert r.entropy.shape == r.mutual_info.shape == r.votes.shape == r.labels_processed.shape == (12, 32, 32)
    assert isinstance(r.quality, StructureAgreement)
    assert np.array_equal(r.quality.voxels, r.counts[:, U.V].cpu().numpy()) and r.quality.voxels.sum() == 12 * 32 * 32
    raw = predict_volume(p, vol, spacing, "ct", crop_size=32, cleanup=False, restore=False, uncertainty=True)
    assert raw.confidence is None and torch.equal(raw.counts, r.counts)        # the counts describe the prediction before the cleanup
    assert np.array_equal(np.bincount(raw.labels.cpu().numpy().ravel(), minlength=len(r.quality.voxels)), r.quality.voxels)
    assert torch.equal(raw.entropy, r.entropy)
