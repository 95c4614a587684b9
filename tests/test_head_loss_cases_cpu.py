"""Pins ``tests/head_loss_cases.py`` without a device: the HW table covers every launch regime, the restatement equals ``coranet_ref`` /
``dtc_ref`` on valid labels, the data-parallel identity holds in fp64, the fp32 replay is finite on every case and meets every bar, and
the comparison helpers reject a reference perturbed the way the bugs they are there for would perturb it."""
import numpy as np
import pytest
import torch

import coranet_ref as CR
import dtc_ref as DR
import head_loss_cases as K


def test_hw_table_covers_every_launch_regime():
    seen = {K.regime(hw) for hw in K.HW_TABLE}
    assert seen == K.REGIMES, (sorted(seen - K.REGIMES), sorted(K.REGIMES - seen))
    assert K.geometry(1) == (1, 1, 1) and K.geometry(512) == (1, 2, 256) and K.geometry(513) == (2, 2, 1)
    assert K.geometry(1300) == (3, 2, 1300 - 768)
    assert K.geometry(65536) == (128, 2, 32768) and K.geometry(65537) == (128, 3, 1) and K.geometry(3 * 65536 + 77) == (128, 7, 77)
    assert K.geometry(512 * 512)[1] == 8                      # the project's 512 x 512 configuration
    ns = {n for hw in K.HW_TABLE for n, _ in K.cora_combos(hw)}
    ls = {L for hw in K.HW_TABLE for _, L in K.cora_combos(hw)}
    assert ns == {1, 2, 3} and ls & {1, 2, 4} and ls - {1, 2, 4}
    for hw in K.HW_TABLE:
        if hw >= K.LARGE:
            assert {L for _, L in K.cora_combos(hw)} == {1, 3} and {c for _, _, c in K.dtc_combos(hw)} == {2, 3}
        for n, b, _ in K.dtc_combos(hw):
            assert b in (1, n - 1, n)
    assert {b - n for hw in K.HW_TABLE for n, b, _ in K.dtc_combos(hw)} >= {0, -1, -2}


@pytest.mark.parametrize("L", [1, 2, 3, 10])
def test_restatement_equals_coranet_ref_on_valid_labels(L):
    c = K.cora_case(3, L, 323, 1)
    z = c.z.double().requires_grad_(True)
    zr = c.z.double().requires_grad_(True)
    got = K.sup_loss(z, c.y, c.w_con, c.w_rad, 0.3, 0.7)
    ref = CR.sup_loss(K.as_nchw(zr), K.as_nchw(c.y), c.w_con, c.w_rad, 0.3, 0.7)
    (-1.7 * got[0]).backward()
    (-1.7 * ref[0]).backward()
    assert torch.allclose(got, ref, rtol=1e-13, atol=0) and torch.allclose(z.grad, zr.grad, rtol=1e-10, atol=1e-18)
    for m in (c.m, torch.from_numpy(np.random.RandomState(2).uniform(size=tuple(c.m.shape))).float()):      # 0/1 and fractional
        z.grad = zr.grad = None
        got = K.semi_loss(z, c.e.double(), c.q, m, 0.7)
        ref = CR.semi_loss(K.as_nchw(zr), K.as_nchw(c.e.double()), K.as_nchw(c.q), K.as_nchw(m), 0.7)
        (-0.6 * got[0] + 0.3 * got[1]).backward()
        (-0.6 * ref[0] + 0.3 * ref[1]).backward()
        assert torch.allclose(got, ref, rtol=1e-13, atol=0) and torch.allclose(z.grad, zr.grad, rtol=1e-10, atol=1e-18)


def test_ignored_labels_add_to_sum_p_only():
    L = 3
    c, v = K.invalid_label_case(2, L, 323), K.cora_case(2, L, 323)
    keep = torch.ones(323, dtype=torch.bool)
    keep[c.planted] = False
    a = K.sup_stats(c.z.double(), c.y, c.w_con, c.w_rad)
    b = K.sup_stats(v.z.double()[:, keep], v.y[:, keep], v.w_con, v.w_rad)               # the same batch without those pixels
    tri_a, tri_b = a[:3 * (L + 1)].view(L + 1, 3), b[:3 * (L + 1)].view(L + 1, 3)
    assert torch.equal(tri_a[:, 2], tri_b[:, 2]) and tri_a[:, 2].sum() == 2 * 320
    assert torch.allclose(tri_a[:, 0], tri_b[:, 0], rtol=1e-13) and torch.allclose(a[-3:], b[-3:], rtol=1e-13)
    extra = torch.softmax(K.head(c.z.double()[:, c.planted], 0, L), -1).sum((0, 1))
    assert torch.allclose(tri_a[:, 1], tri_b[:, 1] + extra, rtol=1e-13)
    # the gradient of such a pixel is the Dice sum_p term alone: no dependence on heads 1 and 2, nor on w_ce
    z = c.z.double().requires_grad_(True)
    K.sup_loss(z, c.y, c.w_con, c.w_rad, 0.5, 0.5)[0].backward()
    g = z.grad[:, c.planted]
    assert not g[..., L + 1:].any() and g[..., :L + 1].abs().min() > 0
    z2 = c.z.double().requires_grad_(True)
    K.sup_loss(z2, c.y, c.w_con, c.w_rad, 0.0, 0.5)[0].backward()
    assert torch.allclose(z2.grad[:, c.planted], g, rtol=1e-12, atol=0)


def test_world_split_identity_in_fp64():
    """Statistics add over ranks; each rank's backward through the GLOBAL statistics, with its own statistics as the only function of
    its logits, is its half of the global gradient (what CoraSupFromStatsFn scales by world ahead of the averaging all-reduce)."""
    L = 4
    c = K.cora_case(4, L, 1300, 2)
    z = c.z.double().requires_grad_(True)
    ref = CR.sup_loss(K.as_nchw(z), K.as_nchw(c.y), c.w_con, c.w_rad, 0.5, 0.5)
    ref[0].backward()
    za, zb = c.z[:2].double().requires_grad_(True), c.z[2:].double().requires_grad_(True)
    sa, sb = K.sup_stats(za, c.y[:2], c.w_con, c.w_rad), K.sup_stats(zb, c.y[2:], c.w_con, c.w_rad)
    for own, other, leaf, half in ((sa, sb, za, z.grad[:2]), (sb, sa, zb, z.grad[2:])):
        out = K.sup_from_stats(own + other.detach(), c.w_con, c.w_rad, float(4 * 1300), 0.5, 0.5)
        out[0].backward()
        assert torch.allclose(out, ref.detach(), rtol=1e-13, atol=0)
        assert torch.allclose(leaf.grad, half, rtol=1e-10, atol=1e-20)


def test_dtc_rows_view_is_dtc_ref():
    t, z, s = DR.loss_case(3, 2, 5, 7, 9, 3)
    rows = lambda x: x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1])
    a = DR.dtc_loss(t.double(), z.double(), s.double(), 1500.0)
    b = DR.dtc_loss(K.as_nchw(rows(t).double()), K.as_nchw(rows(z).double()), K.as_nchw(rows(s).double()), 1500.0)
    assert torch.allclose(a, b, rtol=1e-14, atol=0)


def _self_check_sup(c, combos, tag):
    for (w_dc, w_ce), g in combos:
        (s64, o64, g64), (s32, o32, g32) = K.sup_refs(c, w_ce, w_dc)
        assert all(bool(torch.isfinite(x).all()) for x in (s32, o32, g32)), tag
        K.check_scalars(tag + " stats", s32, s64, s32)
        K.check_scalars(tag + " out", o32, o64, o32)
        K.check_tensor(tag + " grad", np.float32(g) * g32, g * g64, np.float32(g) * g32)


def _self_check_semi(c, combos, tag):
    for gout, cw in combos:
        (s64, o64, g64), (s32, o32, g32) = K.semi_refs(c, gout, cw)
        assert all(bool(torch.isfinite(x).all()) for x in (s32, o32, g32)), tag
        K.check_scalars(tag + " stats", s32, s64, s32)
        K.check_scalars(tag + " out", o32, o64, o32)
        K.check_tensor(tag + " grad", g32, g64, g32)


def _self_check_dtc(c, combos, tag, need_live=True):
    for k, gout in combos:
        (o64, t64, z64), (o32, t32, z32) = K.dtc_refs(c, k, gout)
        assert all(bool(torch.isfinite(x).all()) for x in (o32, t32, z32)), tag
        K.check_scalars(tag + " out", o32, o64, o32)
        K.check_tensor(tag + " gt", t32, t64, t32)
        K.check_tensor(tag + " gz", z32, z64, z32)
        if need_live and gout == (0.0, 1.0):
            assert K.live_share(t64) >= 0.25, (tag, K.live_share(t64))


@pytest.mark.parametrize("hw", K.HW_TABLE)
def test_fp32_replay_is_finite_and_meets_every_bar(hw):
    large = hw >= K.LARGE
    for n, L in K.cora_combos(hw):
        c = K.cora_case(n, L, hw)
        _self_check_sup(c, K.SUP_COMBOS_LARGE if large else K.SUP_COMBOS, f"sup hw{hw} N{n} L{L}")
        _self_check_semi(c, K.SEMI_COMBOS_LARGE if large else K.SEMI_COMBOS, f"semi hw{hw} N{n} L{L}")
    for n, b, cc in K.dtc_combos(hw):
        _self_check_dtc(K.dtc_case(n, b, cc, hw), K.DTC_COMBOS_LARGE if large else K.DTC_COMBOS, f"dtc hw{hw} N{n} B{b} C{cc}")


def test_fp32_replay_on_every_class_count_and_special_case():
    for L in range(1, 11):
        _self_check_sup(K.cora_case(2, L, 1300), K.SUP_COMBOS[:2], f"sup L{L}")
        _self_check_semi(K.cora_case(2, L, 1300), K.SEMI_COMBOS[3:4], f"semi L{L}")
    for cc in range(1, 17):
        _self_check_dtc(K.dtc_case(2, 1, cc, 1300), K.DTC_COMBOS[1:3], f"dtc C{cc}")
    for L in (1, 3, 4, 10):
        for c, tag in ((K.saturated_case(2, L, 1300), "saturated"), (K.all_background_case(L), "all background"),
                       (K.invalid_label_case(2, L, 1300), "invalid labels"), (K.per_sample_case(L), "per sample"),
                       (K.cora_case(2, L, 1300, mask="uniform"), "fractional mask")):
            _self_check_sup(c, K.SUP_COMBOS[:2], f"{tag} sup L{L}")
            _self_check_semi(c, K.SEMI_COMBOS[:4], f"{tag} semi L{L}")
    for cc in (1, 2, 3, 5, 16):
        _self_check_dtc(K.dtc_planted_t_case(cc), K.DTC_COMBOS, f"planted t C{cc}", need_live=False)
        _self_check_dtc(K.dtc_saturated_case(cc), K.DTC_COMBOS, f"saturated z C{cc}", need_live=False)


def test_special_cases_are_what_they_claim():
    for L in (1, 3, 4, 10):
        c = K.per_sample_case(L)
        st = K.semi_stats(c.z.double(), c.e.double(), c.q, c.m)
        base = 3 * (L + 1)
        assert st[0, 3 * L + 2] == 0 and st[1, 3 * L + 2] > 0                       # sample 0 lacks class L in q
        assert st[1, base + 1] == 1300 and st[1, base + 3] == 0 and st[1, base + 2] == 0
        assert st[2, base + 1] == 0 and st[2, base + 3] == 1300 and st[2, base] == 0
        s = K.saturated_case(2, L, 1300)
        p = s.planted
        assert len(p) == 4 and p[0] == 1299 and torch.equal(s.z[:, p[3]], s.e[:, p[3]]) and torch.equal(s.y[:, p[1]], s.q[:, p[1]])
        for n in range(2):
            for k in range(3):
                h = K.head(s.z[n, p[1]], k, L)
                assert h.max() == 80.0 and h[int(s.y[n, p[1]])] == -80.0
        b = K.all_background_case(L)
        tri = K.sup_stats(b.z.double(), b.y, b.w_con, b.w_rad)[:base].view(L + 1, 3)
        assert not tri[1:, [0, 2]].any() and tri[1:, 1].max() < 1e-60                # sum_p = 64 exp(-160): 0 in fp32
        iv = K.invalid_label_case(2, L, 1300)
        assert iv.planted[0] == 1299 and sorted(set(iv.y[0, iv.planted].tolist())) == [-1, L + 1, 1000]
    t = K.dtc_planted_t_case(5).t
    for v in K.PLANTED_T:
        bits = torch.tensor(v).view(torch.int32)
        assert all(bool((t[..., ch].contiguous().view(torch.int32) == bits).any()) for ch in range(5)), v


@pytest.mark.parametrize("L", K.PSEUDO_L)
def test_pseudo_cases(L):
    z = K.pseudo_case(257, L)
    q, m = K.pseudo_ref(z)
    h = [K.head(z, k, L) for k in range(3)]
    assert torch.equal(q, torch.argmax(h[0], 1)) and torch.equal(m, (torch.argmax(h[1], 1) == torch.argmax(h[2], 1)).float())
    assert q[256] == 0 and m[256] == 1                        # the background wins its tie with the last class, in every head
    assert q[0] == 1                                          # two foreground classes tie: the lower index
    assert torch.argmax(h[1][7]) == L and m[7] == (1.0 if torch.argmax(h[2][7]) == L else 0.0)       # NaN wins
    assert q[13] == 0 and m[13] == 1                          # NaN in the shared background: class 0 in every head
    assert q[21] == 0 and m[21] == 0 and q[34] == 0 and q[55] == 0
    assert 0.0 < m.mean() < 1.0 and len(set(q.tolist())) == L + 1
    assert K.PSEUDO_P[-1] > 2048 * 256 and K.PSEUDO_P[-1] % 256


# ------------------------------------------------------------------------------------------- teeth
def _rejects(fn, *a):
    with pytest.raises(AssertionError):
        fn("teeth", *a)


def test_helpers_reject_the_bugs_they_are_there_for():
    c = K.cora_case(2, 3, 1300)
    (s64, o64, g64), (s32, o32, g32) = K.sup_refs(c, 0.5, 0.5)
    K.check_tensor("sanity", g32, g64, g32)
    _rejects(K.check_tensor, g64 / 2, g64, g32)                                     # a gradient scaled by 1 / world
    _rejects(K.check_tensor, g64, -1.7 * g64, np.float32(-1.7) * g32)               # gout ignored
    _rejects(K.check_tensor, torch.zeros_like(g64), g64, g32)
    _rejects(K.check_tensor, g64, torch.zeros_like(g64), torch.zeros_like(g32))     # a structural zero that is not
    small = g64.abs() < 1e-4 * g64.abs().max()                                      # an error on the small gradients alone: the old
    wrong = torch.where(small, 1.05 * g64, g64)                                     # bar (2e-5 of the maximum) lets 5 % of them pass
    assert float((wrong - g64).abs().max() / g64.abs().max()) < 2e-5
    _rejects(K.check_tensor, wrong, g64, g32)
    # a wrong Dice weight (1 / L against 1 / (N L) on the per-sample term) moves a scalar far outside the bar
    _rejects(K.check_scalars, o64 * (1 + 1e-5), o64, o32)

    # one pixel of the last trip dropped from the statistics: 65 537 pixels, the third trip is that pixel alone
    c = K.cora_case(2, 1, 65537)
    assert K.geometry(65537)[1:] == (3, 1)
    full64, full32 = K.sup_stats(c.z.double(), c.y, c.w_con, c.w_rad), K.sup_stats(c.z, c.y, c.w_con, c.w_rad)
    less = K.sup_stats(c.z.double()[:, :-1], c.y[:, :-1], c.w_con, c.w_rad)
    K.check_scalars("sanity", full32, full64, full32)
    cnt = [3 * k + 2 for k in range(2)]
    K.check_counts("sanity", full32[cnt], full64[cnt])
    _rejects(K.check_counts, less[cnt], full64[cnt])
    _rejects(K.check_scalars, less, full64, full32)
    s64s, s32s = K.semi_stats(c.z.double(), c.e.double(), c.q, c.m), K.semi_stats(c.z, c.e, c.q, c.m)
    _rejects(K.check_scalars, K.semi_stats(c.z.double()[:, :-1], c.e.double()[:, :-1], c.q[:, :-1], c.m[:, :-1]), s64s, s32s)
    d = K.dtc_case(2, 1, 2, 65537)
    (o64d, _, _), (o32d, _, _) = K.dtc_refs(d, 1.0, (1.0, 1.0))
    cut = DR.dtc_loss(K.as_nchw(d.t.double()[:, :-1]), K.as_nchw(d.z.double()[:, :-1]), K.as_nchw(d.sdf.double()[:, :-1]), 1.0)
    _rejects(K.check_scalars, cut * (65536 / 65537), o64d, o32d)                    # (the means still divide by all pixels)

    # eps left out of the Dice denominator: visible where a class is absent from labels and prediction alike
    for L in (1, 4, 10):
        b = K.all_background_case(L)
        good64 = K.sup_loss(b.z.double(), b.y, b.w_con, b.w_rad, 0.5, 0.5)
        good32 = K.sup_loss(b.z, b.y, b.w_con, b.w_rad, 0.5, 0.5)
        K.check_scalars("sanity", good32, good64, good32)
        _rejects(K.check_scalars, K.sup_loss(b.z.double(), b.y, b.w_con, b.w_rad, 0.5, 0.5, eps=0.0), good64, good32)
        good64, good32 = K.semi_loss(b.z.double(), b.e.double(), b.q, b.m, 0.7), K.semi_loss(b.z, b.e, b.q, b.m, 0.7)
        _rejects(K.check_scalars, K.semi_loss(b.z.double(), b.e.double(), b.q, b.m, 0.7, eps=0.0), good64, good32)

    # EMA: a kernel that read a truncated alpha (bf16) is outside two roundings
    gen = torch.Generator().manual_seed(9)
    e, p = [torch.randn(100, generator=gen)], [torch.randn(100, generator=gen)]
    ref, bar = K.ema_refs(e, p, 0.99)[0]
    assert np.all(np.abs((e[0] * np.float32(0.99) + p[0] * np.float32(1 - 0.99)).double().numpy() - ref) <= bar)
    assert np.any(np.abs(0.98828125 * e[0].double().numpy() + (1 - 0.98828125) * p[0].double().numpy() - ref) > bar)
