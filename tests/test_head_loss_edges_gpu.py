"""The CoraNet head kernels (``csrc/coranet.hip``) and the loss half of ``csrc/dtc.hip`` against fp64 at the shapes and values where they
take another path: one pixel, a partial / exact / one-past wave, a full block, a thread's second trip, ragged blocks, the 128-block cap
with two, three and seven trips, every class count of both the compile-time and the runtime forms, saturated softmaxes, labels outside
``[0, L]``, non-unit upstream gradients, NaN-filled workspaces and guard bands behind every buffer.  Mostly at the C ABI with raw
buffers (``_hip.call``), so that buffer sizes are exactly what the ``*_ws`` entry points promise.

Cases, references and bars: ``tests/head_loss_cases.py`` (its docstring states every bar; all come from the fp64 / fp32 references,
none from the device).  Every comparison prints ``err``, the bar and ``err / bar``; the worst ratio per family is in DESIGN.md section 5."""
import numpy as np
import pytest
import torch

import head_loss_cases as K

pytestmark = pytest.mark.gpu

SENT = 12345.0
GUARD = 256
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    import smsut_amd  # noqa: F401
    from smsut_amd import ops as o
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return o


@pytest.fixture(scope="module")
def H():
    import smsut_amd  # noqa: F401
    from smsut_amd import _hip
    return _hip


def poisoned(n, dtype=torch.float32, fill=NAN):
    """n elements of ``fill`` (NaN: a word that is read but never written shows) followed by a sentinel guard in the same allocation"""
    buf = torch.full((int(n) + GUARD,), fill, dtype=dtype, device="cuda")
    buf[int(n):] = SENT
    return buf, buf[int(n):]


def untouched(*guards):
    return all(bool((g == SENT).all()) for g in guards)


def gout_buf(*vals):
    """the upstream gradient followed by NaN: the backward must read the leading elements alone"""
    return torch.tensor(list(vals) + [NAN] * (4 - len(vals)), device="cuda")


def dev(c, *names):
    return [getattr(c, k).cuda().contiguous() for k in names]


def worst():
    print("worst err/bar so far:", {k: round(v, 4) for k, v in sorted(K.WORST.items())})


# ------------------------------------------------------------------------------------------- supervised head loss
def sup_stats_call(H, c, z, y, wc, wr, fill):
    L, ns = c.L, 3 * (c.L + 1) + 3
    ws, wg = poisoned(H.call("smsut_cora_ws", c.n, c.hw, L), fill=fill)
    stats, sg = poisoned(ns)
    H.call("smsut_cora_sup_stats", z, y, wc, wr, stats, ws, c.n, c.hw, L, H.stream_ptr())
    assert untouched(wg, sg), "smsut_cora_sup_stats wrote behind its workspace or statistics"
    return stats[:ns].clone()


def run_sup(H, c, combos, tag, family="cora_sup", exact_counts=True):
    """stats / final / bwd of one case at the C ABI; returns the device statistics"""
    L, n, hw = c.L, c.n, c.hw
    z, y, wc, wr = dev(c, "z", "y", "w_con", "w_rad")
    stats = sup_stats_call(H, c, z, y, wc, wr, NAN)
    assert torch.equal(stats, sup_stats_call(H, c, z, y, wc, wr, 0.0)), "the statistics depend on what the workspace held"
    assert not bool(torch.isnan(stats).any()), "a block partial was read but never written"
    done = set()
    for (w_dc, w_ce), g in combos:
        (s64, o64, g64), (s32, o32, g32) = K.sup_refs(c, w_ce, w_dc)
        if not done:
            cnt = [3 * k + 2 for k in range(L + 1)]
            if exact_counts:
                K.check_counts(tag + " counts", stats[cnt].cpu(), s64[cnt])
            K.check_scalars(tag + " stats", stats.cpu(), s64, s32, family + "_stats")
        out, og = poisoned(4)
        H.call("smsut_cora_sup_final", stats, wc, wr, out, L, float(n * hw), w_dc, w_ce, H.stream_ptr())
        K.check_scalars(f"{tag} out w{(w_dc, w_ce)}", out[:4].cpu(), o64, o32, family + "_out")
        for gv in (g, 0.0) if not done else (g,):
            gl, gg = poisoned(n * hw * (3 * L + 1))
            H.call("smsut_cora_sup_bwd", z, y, stats, wc, wr, gout_buf(gv), gl, n, hw, L, float(n * hw), w_dc, w_ce, H.stream_ptr())
            got = gl[:n * hw * (3 * L + 1)].view(n, hw, 3 * L + 1).cpu()
            assert untouched(og, gg), "a guard band was written"
            if gv == 0.0:
                assert bool(torch.isfinite(got).all()) and not bool(got.any()), "gout[0] = 0 must give all zeros"
            else:
                K.check_tensor(f"{tag} grad w{(w_dc, w_ce)} gout {gv}", got, gv * g64, np.float32(gv) * g32, family + "_grad")
        done.add(1)
    return stats


@pytest.mark.parametrize("hw", K.HW_TABLE)
def test_cora_sup_over_the_shape_table(H, hw):
    for n, L in K.cora_combos(hw):
        run_sup(H, K.cora_case(n, L, hw), K.SUP_COMBOS_LARGE if hw >= K.LARGE else K.SUP_COMBOS, f"sup hw{hw} N{n} L{L}")
    worst()


@pytest.mark.parametrize("L", range(1, 11))
def test_cora_sup_every_class_count(H, L):
    run_sup(H, K.cora_case(2, L, 1300), K.SUP_COMBOS[:2], f"sup L{L}")
    worst()


# ------------------------------------------------------------------------------------------- pseudo-labelled head loss
def semi_stats_call(H, c, z, e, q, m, fill):
    ns = 3 * (c.L + 1) + 4
    ws, wg = poisoned(H.call("smsut_cora_ws", c.n, c.hw, c.L), fill=fill)
    stats, sg = poisoned(c.n * ns)
    H.call("smsut_cora_semi_stats", z, e, q, m, stats, ws, c.n, c.hw, c.L, H.stream_ptr())
    assert untouched(wg, sg), "smsut_cora_semi_stats wrote behind its workspace or statistics"
    return stats[:c.n * ns].clone()


def run_semi(H, c, combos, tag, family="cora_semi", exact_counts=True, binary_mask=True):
    L, n, hw = c.L, c.n, c.hw
    ns, base = 3 * (L + 1) + 4, 3 * (L + 1)
    z, e, q, m = dev(c, "z", "e", "q", "m")
    stats = semi_stats_call(H, c, z, e, q, m, NAN)
    assert torch.equal(stats, semi_stats_call(H, c, z, e, q, m, 0.0)), "the statistics depend on what the workspace held"
    assert not bool(torch.isnan(stats).any()), "a block partial was read but never written"
    first = True
    for gout, cw in combos:
        (s64, o64, g64), (s32, o32, g32) = K.semi_refs(c, gout, cw)
        if first:
            exact = ([3 * k + 2 for k in range(L + 1)] if exact_counts else []) + ([base + 1, base + 3] if binary_mask else [])
            if exact:
                K.check_counts(tag + " counts", stats.view(n, ns)[:, exact].cpu(), s64[:, exact])
            K.check_scalars(tag + " stats", stats.cpu(), s64, s32, family + "_stats")
        out, og = poisoned(2)
        H.call("smsut_cora_semi_final", stats, out, n, L, cw, H.stream_ptr())
        K.check_scalars(f"{tag} out cw{cw}", out[:2].cpu(), o64, o32, family + "_out")
        gz, gg = poisoned(n * hw * (3 * L + 1))
        H.call("smsut_cora_semi_bwd", z, e, q, m, stats, gout_buf(*gout), gz, n, hw, L, cw, H.stream_ptr())
        got = gz[:n * hw * (3 * L + 1)].view(n, hw, 3 * L + 1).cpu()
        assert untouched(og, gg), "a guard band was written"
        K.check_tensor(f"{tag} grad gout {gout} cw{cw}", got, g64, g32, family + "_grad")
        if gout[0] == 0.0:
            assert not bool(got[c.m == 1].any()), "with gout = (0, .) a pixel with m == 1 gets exactly 0 in every channel"
        first = False
    return stats


@pytest.mark.parametrize("hw", K.HW_TABLE)
def test_cora_semi_over_the_shape_table(H, hw):
    for n, L in K.cora_combos(hw):
        run_semi(H, K.cora_case(n, L, hw), K.SEMI_COMBOS_LARGE if hw >= K.LARGE else K.SEMI_COMBOS, f"semi hw{hw} N{n} L{L}")
    worst()


@pytest.mark.parametrize("L", range(1, 11))
def test_cora_semi_every_class_count(H, L):
    run_semi(H, K.cora_case(2, L, 1300), K.SEMI_COMBOS[3:4] + K.SEMI_COMBOS[1:2], f"semi L{L}")
    worst()


@pytest.mark.parametrize("L", [1, 3, 4, 10])
def test_cora_semi_per_sample_statistics_and_fractional_mask(H, L):
    """N = 3 with a class missing from q in sample 0, m == 1 in sample 1 and m == 0 in sample 2: a per-sample statistic that lands in
    another sample's row, or a batch-wide Dice, shows.  Then a mask drawn from [0, 1] (the formulas are linear in m)."""
    c = K.per_sample_case(L)
    stats = run_semi(H, c, K.SEMI_COMBOS[:4], f"per-sample L{L}").view(3, -1).cpu()
    base = 3 * (L + 1)
    assert stats[0, 3 * L + 2] == 0 and stats[0, 3 * L] == 0                          # count and tp of the missing class
    assert stats[1, base + 2] == 0 and stats[1, base + 3] == 0 and stats[2, base] == 0 and stats[2, base + 1] == 0
    run_semi(H, K.cora_case(2, L, 1300, mask="uniform"), K.SEMI_COMBOS[:4], f"fractional mask L{L}", binary_mask=False)
    worst()


# ------------------------------------------------------------------------------------------- saturation, ignored labels
@pytest.mark.parametrize("L", [1, 3, 4, 10])
def test_cora_saturated_logits(H, L):
    """25 * randn and the planted pixels of ``saturated_case``; then every pixel background by 160, where the Dice coefficient of each
    (absent) foreground class is smooth / (smooth + eps)."""
    c = K.saturated_case(2, L, 1300)
    run_sup(H, c, K.SUP_COMBOS[:2], f"saturated sup L{L}", "cora_sup_saturated")
    stats = run_semi(H, c, K.SEMI_COMBOS[:4], f"saturated semi L{L}", "cora_semi_saturated")
    # The unmasked pixel where student == teacher bit for bit: its MSE gradient (gout = (0, 1)) is 0 in exact arithmetic.  On the device
    # it is 0 up to the rounding of one multiply: the library is built with -ffp-contract=fast, and `p_z - pe * inv` of the teacher's
    # softmax contracts into one fma, which leaves the rounding residual of `pe * inv` (measured: up to 1e-12 at a gradient scale of
    # 4.5e-4).  Bound per head: |d_c| <= 2^-23 p_c, |dk| = |sum_c p_c d_c| <= 2^-23, so |p_c (d_c - dk)| <= 2^-22; channel 0 sums three heads.
    z, e, q, m = dev(c, "z", "e", "q", "m")
    gz, gg = poisoned(c.z.numel())
    H.call("smsut_cora_semi_bwd", z, e, q, m, stats, gout_buf(0.0, 1.0), gz, 2, 1300, L, 0.7, H.stream_ptr())
    got = gz[:c.z.numel()].view(2, 1300, 3 * L + 1).cpu()
    fu = 0.7 * (2.0 / 3.0) / float((1 - c.m).sum())
    resid = float(got[:, c.planted[3]].abs().max())
    print(f"saturated semi L{L}: student == teacher pixel, |gradient| {resid:.3g}, bound {3 * fu * 2.0 ** -22:.3g}")
    assert untouched(gg) and resid <= 3 * fu * 2.0 ** -22 and float(got[c.m == 0].abs().max()) > 1e-2 * fu
    b = K.all_background_case(L)
    run_sup(H, b, K.SUP_COMBOS[:2], f"all-background sup L{L}", "cora_sup_saturated")
    run_semi(H, b, K.SEMI_COMBOS[:4], f"all-background semi L{L}", "cora_semi_saturated")
    worst()


@pytest.mark.parametrize("L", [1, 3, 4, 10])
def test_cora_labels_outside_the_range(H, L):
    """-1, L + 1 and 1000 in labels and pseudo labels (the last pixel among them): such a pixel adds to sum_p only -- no tp, no count,
    no CE term in any head, CE(h0) still divided by N * HW -- and its gradient is the Dice sum_p term alone."""
    c = K.invalid_label_case(2, L, 1300)
    stats = run_sup(H, c, K.SUP_COMBOS[:2], f"ignored labels sup L{L}", "cora_ignored")
    assert float(stats[[3 * k + 2 for k in range(L + 1)]].sum()) == 2 * 1300 - 6
    run_semi(H, c, K.SEMI_COMBOS[:4], f"ignored labels semi L{L}", "cora_ignored")
    # (w_dc, w_ce) = (0, 1): no Dice term, so an ignored pixel's gradient is exactly 0 in every channel
    z, y, wc, wr = dev(c, "z", "y", "w_con", "w_rad")
    gl, gg = poisoned(2 * 1300 * (3 * L + 1))
    H.call("smsut_cora_sup_bwd", z, y, stats, wc, wr, gout_buf(-1.7), gl, 2, 1300, L, 2600.0, 0.0, 1.0, H.stream_ptr())
    got = gl[:2 * 1300 * (3 * L + 1)].view(2, 1300, 3 * L + 1)[:, c.planted].cpu()
    assert untouched(gg) and bool(torch.isfinite(got).all()) and not bool(got.any())
    worst()


# ------------------------------------------------------------------------------------------- pseudo labels
@pytest.mark.parametrize("L", K.PSEUDO_L)
@pytest.mark.parametrize("p", K.PSEUDO_P)
def test_cora_pseudo_is_exact(H, p, L):
    z = K.pseudo_case(p, L)
    q, qg = poisoned(p, torch.int64, fill=-7)
    m, mg = poisoned(p)
    H.call("smsut_cora_pseudo", z.cuda(), q, m, p, L, H.stream_ptr())
    rq, rm = K.pseudo_ref(z)
    assert untouched(qg, mg)
    assert torch.equal(q[:p].cpu(), rq) and torch.equal(m[:p].cpu(), rm)


# ------------------------------------------------------------------------------------------- EMA
def test_ema_update_chunks_tables_and_guards(ops):
    """Every tensor is a view one float into its own guarded buffer: a chunk that starts or ends a float off, or an entry of the table
    that points at a neighbour, lands in a guard.  Lengths around the 8192-element chunk, and 300 tensors of 3 (many table entries)."""
    rs = np.random.RandomState(5)

    def guarded(n):
        buf = torch.full((n + 1 + GUARD,), SENT, device="cuda")
        buf[1:1 + n] = torch.from_numpy(rs.standard_normal(n)).float().cuda()
        return buf, buf[1:1 + n]

    ebufs, ema = zip(*[guarded(n) for n in K.EMA_LENGTHS])
    pbufs, par = zip(*[guarded(n) for n in K.EMA_LENGTHS])
    e0, p0 = [e.cpu().clone() for e in ema], [p.cpu().clone() for p in par]

    def guards_intact():
        return all(bool((b[:1] == SENT).all()) and bool((b[1 + n:] == SENT).all()) for bufs in (ebufs, pbufs)
                   for b, n in zip(bufs, K.EMA_LENGTHS))

    ops.ema_update(ema, par, 1.0)
    assert all(torch.equal(e.cpu(), r) for e, r in zip(ema, e0)), "alpha = 1 leaves ema bit-equal"
    ops.ema_update(ema, par, 0.99)
    ratio = 0.0
    for e, (ref, bar) in zip(ema, K.ema_refs(e0, p0, 0.99)):
        err = np.abs(e.cpu().double().numpy() - ref)
        assert np.all(err <= bar), (len(ref), float((err / bar).max()))
        ratio = max(ratio, float((err / bar).max()))
    print(f"ema: worst err/bar {ratio:.3g}")
    assert guards_intact() and all(torch.equal(p.cpu(), r) for p, r in zip(par, p0))
    ops.ema_update(ema, par, 0.0)
    assert all(torch.equal(e, p) for e, p in zip(ema, par)), "alpha = 0 gives p bit for bit"
    assert guards_intact()


# ------------------------------------------------------------------------------------------- through ops
def nchw_dev(rows, h, w, channels_last=True):
    """rows [N, HW, C] as a logical NCHW device tensor, over NHWC memory or NCHW-contiguous"""
    t = rows.cuda().view(rows.shape[0], h, w, -1).permute(0, 3, 1, 2)
    return t if channels_last else t.contiguous()


def test_cora_sup_world_2_without_a_second_process(ops):
    """The data-parallel branch of CoraSupFromStatsFn: each half batch with the SUM of both halves' statistics (what the all-reduce
    leaves) and world = 2 returns the global-batch loss, and its gradient / 2 is its half of the global gradient."""
    L, h, w = 4, 20, 65
    c = K.cora_case(4, L, h * w, 2)
    (s64, o64, g64), (s32, o32, g32) = K.sup_refs(c, 0.5, 0.5)
    wc, wr = c.w_con.cuda(), c.w_rad.cuda()
    zs = [nchw_dev(c.z[i:i + 2], h, w).requires_grad_(True) for i in (0, 2)]
    ys = [c.y[i:i + 2].view(2, h, w).cuda() for i in (0, 2)]
    stats = ops.cora_sup_stats(zs[0], ys[0], wc, wr) + ops.cora_sup_stats(zs[1], ys[1], wc, wr)
    K.check_scalars("world 2 summed stats", stats.cpu(), s64, s32, "cora_world2")
    for i in (0, 1):
        out = ops.CoraSupFromStatsFn.apply(zs[i], ys[i], stats, wc, wr, 0.5, 0.5, 2)
        K.check_scalars(f"world 2 out of half {i}", out.detach().cpu(), o64, o32, "cora_world2")
        out[0].backward()
        got = (zs[i].grad / 2).permute(0, 2, 3, 1).reshape(2, h * w, -1)
        K.check_tensor(f"world 2 grad of half {i}", got, g64[2 * i:2 * i + 2], g32[2 * i:2 * i + 2], "cora_world2")
    worst()


def test_nchw_contiguous_logits_give_the_same_bits(ops):
    L, h, w = 3, 20, 65
    c = K.cora_case(2, L, h * w)
    wc, wr = c.w_con.cuda(), c.w_rad.cuda()
    y, q, m = (t.view(2, h, w).cuda() for t in (c.y, c.q, c.m))
    res = []
    for channels_last in (True, False):
        z = nchw_dev(c.z, h, w, channels_last).requires_grad_(True)
        e = nchw_dev(c.e, h, w, channels_last)
        assert z.is_contiguous() != channels_last
        sup = ops.cora_sup_loss(z, y, wc, wr, 0.5, 0.5)
        semi = ops.cora_semi_loss(z, e, q, m, 0.7)
        (-1.7 * sup[0] - 0.6 * semi[0] + 0.3 * semi[1]).backward()
        res.append((sup.detach(), semi.detach(), z.grad.contiguous(), *ops.cora_pseudo(z)))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------- DTC loss
def dtc_fwd_call(H, c, t, z, s, k, fill):
    nd = H.call("smsut_dtc_ws", c.n, c.hw) // 2                       # the workspace holds doubles
    assert H.call("smsut_dtc_ws", c.n, c.hw) == 4 * c.n * K.blocks(c.hw)
    ws, wg = poisoned(nd, torch.float64, fill=fill)
    out, og = poisoned(2)
    H.call("smsut_dtc_loss_fwd", t, z, s, out, ws, c.n, c.b, c.hw, c.c, k, H.stream_ptr())
    assert untouched(wg, og), "smsut_dtc_loss_fwd wrote behind its workspace or output"
    return out[:2].clone()


def run_dtc(H, c, combos, tag, family="dtc", need_live=True):
    n, b, cc, hw = c.n, c.b, c.c, c.hw
    t, z, s = dev(c, "t", "z", "sdf")
    outs = {}
    for k, gout in combos:
        (o64, t64, z64), (o32, t32, z32) = K.dtc_refs(c, k, gout)
        if k not in outs:
            outs[k] = dtc_fwd_call(H, c, t, z, s, k, NAN)
            assert torch.equal(outs[k], dtc_fwd_call(H, c, t, z, s, k, 0.0)), "the loss depends on what the workspace held"
            K.check_scalars(f"{tag} out k{k}", outs[k].cpu(), o64, o32, family + "_out")
        gt, tg = poisoned(n * hw * cc)
        gz, zg = poisoned(n * hw * cc)
        H.call("smsut_dtc_loss_bwd", t, z, s, gout_buf(*gout), gt, gz, n, b, hw, cc, k, H.stream_ptr())
        assert untouched(tg, zg), "smsut_dtc_loss_bwd wrote behind a gradient"
        got_t, got_z = gt[:n * hw * cc].view(n, hw, cc).cpu(), gz[:n * hw * cc].view(n, hw, cc).cpu()
        K.check_tensor(f"{tag} gt k{k} gout {gout}", got_t, t64, t32, family + "_gt")
        K.check_tensor(f"{tag} gz k{k} gout {gout}", got_z, z64, z32, family + "_gz")
        if gout[1] == 0.0:
            assert not bool(got_z.any()) and not bool(got_t[b:].any()), "gout = (., 0): gz and the unlabelled slices of gt are 0"
        if need_live and gout == (0.0, 1.0) and k == 1500.0:
            assert K.live_share(t64) >= 0.25, (tag, K.live_share(t64))
    return outs


@pytest.mark.parametrize("hw", K.HW_TABLE)
def test_dtc_loss_over_the_shape_table(H, hw):
    for n, b, cc in K.dtc_combos(hw):
        run_dtc(H, K.dtc_case(n, b, cc, hw), K.DTC_COMBOS_LARGE if hw >= K.LARGE else K.DTC_COMBOS, f"dtc hw{hw} N{n} B{b} C{cc}")
    worst()


@pytest.mark.parametrize("cc", range(1, 17))
def test_dtc_loss_every_channel_count(H, cc):
    run_dtc(H, K.dtc_case(2, 1, cc, 1300), K.DTC_COMBOS[1:3], f"dtc C{cc}")
    worst()


@pytest.mark.parametrize("cc", [1, 2, 3, 5, 16])
def test_dtc_loss_planted_t_and_saturated_z(H, cc):
    """t = +-0, +-1, +-1e-30, +-0.0592 (|k t| = 88.8: exp reaches the fp32 denormals) in every channel; then logits 25 * randn with
    pixels decided by 160 and an all-equal one.  Everything finite and within the bars."""
    run_dtc(H, K.dtc_planted_t_case(cc), K.DTC_COMBOS, f"planted t C{cc}", "dtc_planted_t", need_live=False)
    run_dtc(H, K.dtc_saturated_case(cc), K.DTC_COMBOS, f"saturated z C{cc}", "dtc_saturated_z", need_live=False)
    worst()


@pytest.mark.parametrize("cc", [2, 3])
def test_dtc_loss_sdf_equal_to_t_and_reproducibility(H, cc):
    c = K.clone_case(K.dtc_case(3, 2, cc, 1300, 6))
    c.sdf = c.t[:2].clone()                                            # the first term and its gradient are exactly 0
    outs = run_dtc(H, c, K.DTC_COMBOS[:1], f"sdf = t[:B] C{cc}", need_live=False)
    assert outs[1500.0][0].item() == 0.0
    t, z, s = dev(c, "t", "z", "sdf")
    gt, _ = poisoned(3 * 1300 * cc)
    gz, _ = poisoned(3 * 1300 * cc)
    H.call("smsut_dtc_loss_bwd", t, z, s, gout_buf(1.0, 0.0), gt, gz, 3, 2, 1300, cc, 1500.0, H.stream_ptr())
    assert not bool(gt[:3 * 1300 * cc].any()) and not bool(gz[:3 * 1300 * cc].any())
    # two runs, bit-identical (a NaN-filled against a zero-filled workspace is part of every run_dtc)
    c = K.dtc_case(2, 2, cc, 3 * 65536 + 77)
    t, z, s = dev(c, "t", "z", "sdf")
    runs = []
    for _ in range(2):
        out = dtc_fwd_call(H, c, t, z, s, 1500.0, NAN)
        gt, _ = poisoned(c.t.numel())
        gz, _ = poisoned(c.t.numel())
        H.call("smsut_dtc_loss_bwd", t, z, s, gout_buf(0.3, 0.7), gt, gz, 2, 2, c.hw, cc, 1500.0, H.stream_ptr())
        runs.append((out, gt.clone(), gz.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
