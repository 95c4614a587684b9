"""``smsut_eval_overlap`` / ``ops.eval_overlap`` (csrc/evaluate.hip) against a NumPy restatement written here.  Everything is
integers or bytes, so every comparison is exact equality.

Shapes: HW = 1, 63, 64, 65, 255, 256, 257, 2000 (one pixel, around a wave, around the 256-pixel tile, several tiles; the row
length 5 * HW is not a multiple of 4 at HW = 63, so slices start off a 16-byte boundary) and 129 x 130 = 16770 pixels = 66 tiles,
more than the 64 workgroups a slice gets, so some workgroups walk two tiles.  Layouts (C, K): (2, 2), (5, 5) compile-time class counts;
(13, 5) CoraNet's head 0; (32, 32) the runtime class loop; (40, 5), (36, 6) rows too long for the LDS staging, read in place."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16), (1, 257), (40, 50)]
LAYOUTS = [(2, 2), (5, 5), (13, 5), (32, 32)]
EXTRA = [((129, 130), (5, 5)), ((129, 130), (13, 5)), ((129, 130), (32, 32)), ((7, 9), (40, 5)), ((40, 50), (40, 5)), ((40, 50), (36, 6)),
         ((129, 130), (36, 6))]
CASES = [(s, l) for s in SHAPES for l in LAYOUTS] + EXTRA
N, V, PRE, SENTINEL = 3, 4, 2 ** 40, 0xEE
IDS_A, IDS_B = [2, 2, 0], [0, -1, 3]          # two slices in one volume + a second volume | a skipped slice; slot 1 is never named


def np_argmax(z, k):
    """First maximum of channels 0 .. k-1, a NaN wins (the kernel's comparison, channel by channel)."""
    best = z[:, 0].copy()
    p = np.zeros(best.shape, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for c in range(1, k):
            v = z[:, c]
            take = (v > best) | (np.isnan(v) & ~np.isnan(best))
            best = np.where(take, v, best)
            p = np.where(take, c, p)
    return p


def np_overlap(z, lab, ids, k, counts, pred):
    """counts [V, k, 3] += {|P & G|, |P|, |G|}; pred [N, H, W] written for the slices that are not skipped."""
    p = np_argmax(z, k)
    for n, v in enumerate(ids):
        if not 0 <= v < counts.shape[0]:
            continue
        pred[n] = p[n]
        for c in range(k):
            counts[v, c, 0] += np.count_nonzero((p[n] == c) & (lab[n] == c))
            counts[v, c, 1] += np.count_nonzero(p[n] == c)
            counts[v, c, 2] += np.count_nonzero(lab[n] == c)
    return p


def make_batch(seed, h, w, c, k, special):
    """Logits [N, c, h, w] and labels [N, h, w] with -1, k and 255 sprinkled in.  ``special``: slice 0 all-equal logits (prediction
    0 everywhere); on slice 1 a NaN in channel min(2, k - 1) of the first pixel and +inf in two channels of the last one."""
    rs = np.random.RandomState(seed)
    z = rs.standard_normal((N, c, h, w)).astype(np.float32)
    lab = rs.randint(0, k, (N, h, w)).astype(np.int64)
    flat = lab.reshape(N, -1)
    for j, bad in enumerate((-1, k, 255)):
        flat[:, (j * 5 + 2) % flat.shape[1]::7] = bad
    if h * w == 1:
        flat[0, 0], flat[1, 0], flat[2, 0] = k, k - 1, -1    # (one pixel per slice: one in-range label, on slice 1)
    if special:
        z[0] = 0.25
        zf = z[1].reshape(c, -1)
        zf[min(2, k - 1), 0] = np.nan
        if h * w > 1:
            zf[0, -1] = zf[k - 1, -1] = np.inf
    return z, lab


def dev_cl(z):
    return torch.from_numpy(z).cuda().contiguous(memory_format=torch.channels_last)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.parametrize("hw,ck", CASES, ids=[f"{s[0]}x{s[1]}-C{l[0]}K{l[1]}" for s, l in CASES])
def test_counts_and_prediction_equal_numpy(hw, ck):
    from smsut_amd import _hip as H, ops
    (h, w), (c, k) = hw, ck
    za, la = make_batch(100 * h + w + c, h, w, c, k, special=True)
    zb, lb = make_batch(100 * h + w + c + 1, h, w, c, k, special=False)
    want_counts = np.full((V, k, 3), PRE, dtype=np.int64)
    want_pred = [np.full((N, h, w), SENTINEL, dtype=np.int64) for _ in range(2)]
    pa = np_overlap(za, la, IDS_A, k, want_counts, want_pred[0])
    np_overlap(zb, lb, IDS_B, k, want_counts, want_pred[1])
    assert (pa[0] == 0).all()                                                  # all-equal logits: class 0 everywhere
    assert pa[1].reshape(-1)[0] == min(2, k - 1)                               # the NaN wins
    assert h * w == 1 or pa[1].reshape(-1)[-1] == 0                            # the first of two +inf wins

    lib, s = H.load(), H.stream_ptr()
    counts = torch.full((V, k, 3), PRE, dtype=torch.int64, device="cuda")
    got_pred = []
    for z, lab, ids in ((za, la, IDS_A), (zb, lb, IDS_B)):
        zd, ld = dev_cl(z), torch.from_numpy(lab).cuda()
        vol = torch.tensor(ids, dtype=torch.int32, device="cuda")
        pred = torch.full((N, h, w), SENTINEL, dtype=torch.uint8, device="cuda")
        assert lib.smsut_eval_overlap(p(zd), p(ld), p(vol), p(counts), p(pred), N, h * w, c, k, V, s) == 0
        got_pred.append(pred.cpu().numpy())
    got = counts.cpu().numpy()
    assert (got == want_counts).all(), (got - PRE, want_counts - PRE)           # two calls add up, on top of 2**40: 64-bit adds
    assert (got[1] == PRE).all()                                               # the volume nobody named
    assert got[0, :, 1].sum() - k * PRE == 2 * h * w and got[3, :, 1].sum() - k * PRE == h * w
    for g_, w_ in zip(got_pred, want_pred):
        assert (g_ == w_).all()
    assert (got_pred[1][1] == SENTINEL).all()                                  # the skipped slice's bytes were never written

    # the prediction is argmax_channels' on the same tensor, byte for value (NaN pixels included)
    zk = dev_cl(za) if k == c else dev_cl(np.ascontiguousarray(za[:, :k]))
    assert (ops.argmax_channels(zk).cpu().numpy() == pa).all()
    assert (got_pred[0][:2] == pa[:2]).all()

    # the Python entry: same counts without the pre-load, the prediction returned, or None
    c2 = torch.zeros(V, k, 3, dtype=torch.int64, device="cuda")
    pr = ops.eval_overlap(dev_cl(za), torch.from_numpy(la).cuda(), IDS_A, c2, classes=None if k == c else k)
    assert pr.dtype == torch.uint8 and (pr.cpu().numpy() == pa).all()
    assert ops.eval_overlap(dev_cl(zb), torch.from_numpy(lb).cuda(), IDS_B, c2, classes=k, want_pred=False) is None
    assert (c2.cpu().numpy() == want_counts - PRE).all()


@pytest.mark.parametrize("hw,ck", [((7, 9), (5, 5)), ((40, 50), (13, 5)), ((15, 17), (32, 32))])
def test_nchw_contiguous_logits_give_the_same_result(hw, ck):
    from smsut_amd import ops
    (h, w), (c, k) = hw, ck
    z, lab = make_batch(7, h, w, c, k, special=True)
    ld = torch.from_numpy(lab).cuda()
    res = []
    for zd in (dev_cl(z), torch.from_numpy(z).cuda().contiguous()):
        cnt = torch.zeros(V, k, 3, dtype=torch.int64, device="cuda")
        res.append((ops.eval_overlap(zd, ld, IDS_A, cnt, classes=k), cnt))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and int(res[0][1].sum()) > 0


def test_invalid_arguments_raise_or_return_minus_one_without_a_launch():
    from smsut_amd import _hip as H, ops
    h = w = 8
    z, lab = make_batch(3, h, w, 5, 5, special=False)
    zd, ld = dev_cl(z), torch.from_numpy(lab).cuda()
    counts = torch.full((V, 5, 3), 17, dtype=torch.int64, device="cuda")
    ok = IDS_A
    with pytest.raises(TypeError):
        ops.eval_overlap(zd.double(), ld, ok, counts)                             # wrong logits dtype
    with pytest.raises(TypeError):
        ops.eval_overlap(zd, ld.int(), ok, counts)                                # wrong label dtype
    with pytest.raises(TypeError):
        ops.eval_overlap(zd, ld, ok, counts.int())                                # wrong counts dtype
    with pytest.raises(TypeError):
        ops.eval_overlap(zd.cpu(), ld, ok, counts)                                # CPU tensors
    with pytest.raises(TypeError):
        ops.eval_overlap(zd, ld.cpu(), ok, counts)
    with pytest.raises(ValueError):
        ops.eval_overlap(dev_cl(np.zeros((N, 40, h, w), np.float32)), ld, ok, torch.zeros(V, 33, 3, dtype=torch.int64, device="cuda"),
                         classes=33)                                              # classes > 32
    with pytest.raises(ValueError):
        ops.eval_overlap(zd, ld, ok, counts, classes=6)                           # classes > C
    with pytest.raises(ValueError):
        ops.eval_overlap(zd, ld, [0, V, 1], counts)                               # an id >= V
    with pytest.raises(ValueError):
        ops.eval_overlap(zd, ld, [0, -2, 1], counts)                              # below -1
    with pytest.raises(ValueError):
        ops.eval_overlap(zd, ld, [0, 1], counts)                                  # length mismatch
    with pytest.raises(ValueError):
        ops.eval_overlap(zd, ld[:, :4], ok, counts)                               # label shape
    with pytest.raises(ValueError):
        ops.eval_overlap(zd, ld, ok, counts[:, :4])                               # counts shape (and not contiguous)

    lib, s = H.load(), H.stream_ptr()
    vol = torch.tensor(ok, dtype=torch.int32, device="cuda")
    pred = torch.full((N, h, w), SENTINEL, dtype=torch.uint8, device="cuda")
    call = lambda n, hw, c, k, v: lib.smsut_eval_overlap(p(zd), p(ld), p(vol), p(counts), p(pred), n, hw, c, k, v, s)
    assert call(N, h * w, 5, 6, V) == -1                                          # K > C
    assert call(N, h * w, 5, 0, V) == -1                                          # K = 0
    assert call(N, 0, 5, 5, V) == -1                                              # HW = 0
    assert call(N, h * w, 5, 5, 0) == -1                                          # V = 0
    assert call(N, h * w, 40, 33, V) == -1                                        # K > 32
    assert call(65536, h * w, 5, 5, V) == -1 and call(-1, h * w, 5, 5, V) == -1   # N out of range
    assert call(0, h * w, 5, 5, V) == 0                                           # nothing to do: fine, and no launch
    torch.cuda.synchronize()
    assert (counts == 17).all() and (pred == SENTINEL).all()                      # none of the above launched anything
    assert call(N, h * w, 5, 5, V) == 0                                           # and the device is fine afterwards
    torch.cuda.synchronize()
    assert int(counts[:, :, 1].sum()) - 17 * V * 5 == N * h * w
