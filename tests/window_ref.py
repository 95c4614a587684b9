"""fp64 restatement of the sliding-window blend (csrc/window.hip) and the cases its tests share.  Host code only.

The blend.  Tile (iy, ix), fp32 ``[N, wh, ww, K]``, lies at rows ``ys[iy]`` .. and columns ``xs[ix]`` .. of the grid ``(H, W)``; its
pixel (i, j) weighs ``wy[i] * wx[j]``.  Per grid pixel the covering tiles' probabilities are averaged with their weights,
``prob_k = sum_t (w_t / sum_j w_j) p_t[k]``: here with every product, quotient and sum in fp64 on the same fp32 inputs (``wy[i] * wx[j]`` of two
fp32 numbers is exact in fp64).

The budget.  The kernel works in fp32 (unit roundoff u = 2^-24) on a pixel under m tiles:
``w_t = fl(wy wx)``, ``s = w_0 + ... + w_{m-1}`` in order, ``v_t = fl(w_t / s)``, ``acc_k = v_0 p_0[k] + ... `` in order.  To first order
v_t carries (m + 1) u of relative error: u from the product, (m - 1) u from the m - 1 additions of a sum of positive terms, u from
the division.  Each accumulated term v_t p_t[k] adds u for its product and takes part in at most m - 1 additions, (m - 1) u; all of
these are relative to terms whose sum ``sum_t v_t p_t[k]`` is at most 1 (probabilities, weights that sum to 1).  That is
(m + 1) + 1 + (m - 1) = 2 m + 1 units; the products' errors also sit inside s, where their weighted mean can add one more:
``budget(m) = 2^-24 (2 m + 2)``, absolute, for ``prob`` and ``conf``, with m the largest cover of the case.  (A fused multiply-add
drops a rounding; under one tile v = w / w = 1 and the kernel is exact.)  If the kernel exceeds it, the kernel is wrong.

``pred`` is compared where the two largest blended probabilities of the reference are at least ``4 budget`` apart (each side may
move by a budget, twice over for safety); the share of pixels this rule leaves out is asserted, not just reported."""
import functools

import numpy as np
import torch


def plan(size, window, overlap):
    """``ops.window_plan`` restated (integer arithmetic)."""
    target = max(1, int(window * (1 - overlap)))
    n = -(-(size - window) // target) + 1
    return (0,) if n == 1 else tuple((i * (size - window)) // (n - 1) for i in range(n))


def weights(n, blend):
    """``ops.window_weights`` restated: fp64, rounded once to fp32."""
    if blend == "constant":
        return np.ones(n, dtype=np.float32)
    i = np.arange(n, dtype=np.float64)
    return np.exp(-0.5 * ((i - (n - 1) / 2) / (n / 8)) ** 2).astype(np.float32)


def budget(m):
    return 2.0 ** -24 * (2 * m + 2)


def first_max(p):
    return torch.argmax((p == p.max(dim=-1, keepdim=True).values).to(torch.uint8), dim=-1)


def blend_ref(tiles, ys, xs, hw, wy, wx):
    """``tiles``: ``len(ys) * len(xs)`` arrays / tensors ``[N, wh, ww, K]`` in row-major (iy, ix) order; ``wy [wh]``, ``wx [ww]``.
    Returns ``(pred [N, H, W] int64, conf [N, H, W], prob [N, H, W, K], gap [N, H, W], cover)``: fp64 but ``pred``; ``gap`` is
    the distance between the two largest blended probabilities (inf with one class), ``cover`` the largest number of tiles over
    one pixel."""
    h, w = hw
    as64 = lambda a: torch.as_tensor(np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)).double()
    tiles = [as64(t) for t in tiles]
    n, wh, ww, k = tiles[0].shape
    assert len(tiles) == len(ys) * len(xs)
    wmap = as64(wy).view(wh, 1) * as64(wx).view(1, ww)
    acc = torch.zeros(n, h, w, k, dtype=torch.float64)
    wsum = torch.zeros(h, w, dtype=torch.float64)
    count = torch.zeros(h, w, dtype=torch.int64)
    for y0 in ys:
        for x0 in xs:
            wsum[y0:y0 + wh, x0:x0 + ww] += wmap
            count[y0:y0 + wh, x0:x0 + ww] += 1
    assert int(count.min()) >= 1, "the plan leaves a pixel uncovered"
    it = iter(tiles)
    for y0 in ys:                                            # normalised before the sum, as the kernel: one tile is w / w = 1
        for x0 in xs:
            acc[:, y0:y0 + wh, x0:x0 + ww] += (wmap / wsum[y0:y0 + wh, x0:x0 + ww]).view(1, wh, ww, 1) * next(it)
    prob = acc
    pred = first_max(prob)
    conf = prob.gather(-1, pred.unsqueeze(-1)).squeeze(-1)
    if k > 1:
        top2 = torch.topk(prob, 2, dim=-1).values
        gap = top2[..., 0] - top2[..., 1]
    else:
        gap = torch.full_like(conf, float("inf"))
    return pred, conf, prob, gap, int(count.max())


# (N, H, W, window, overlap, K, blend, offset views)
CASES = [(2, 40, 52, 24, 0.5, 5, "gaussian", False),       # 3 x 4 tiles, cover 9, uneven steps
         (1, 37, 50, 24, 0.5, 5, "gaussian", True),        # bases 4 bytes past a 16-byte boundary, odd row lengths
         (3, 20, 20, 8, 0.75, 5, "gaussian", False),       # 49 tiles, cover 16
         (1, 33, 35, 16, 0.5, 4, "constant", False),       # even K
         (1, 24, 40, 12, 0.25, 32, "gaussian", False),     # the class limit
         (1, 19, 23, 12, 0.5, 2, "gaussian", True)]
IDS = ["n2-40x52-w24", "37x50-w24-offset", "n3-20x20-w8-49tiles", "33x35-w16-constant-k4", "24x40-w12-k32", "19x23-w12-k2-offset"]


class Case:
    """The inputs of one entry of CASES and their reference, computed once and left unchanged."""

    def __init__(self, spec, rng):
        self.n, self.h, self.w, self.window, self.overlap, self.k, self.blend, self.offset = spec
        self.ys, self.xs = plan(self.h, self.window, self.overlap), plan(self.w, self.window, self.overlap)
        self.wy = self.wx = weights(self.window, self.blend)
        self.tiles = []
        for _ in range(len(self.ys) * len(self.xs)):        # softmaxes of 3 N(0, 1) logits, rounded once to fp32
            z = torch.from_numpy(3.0 * rng.standard_normal((self.n, self.window, self.window, self.k)))
            self.tiles.append(torch.softmax(z, dim=-1).float())
        self.pred, self.conf, self.prob, self.gap, self.cover = blend_ref(self.tiles, self.ys, self.xs, (self.h, self.w), self.wy,
                                                                          self.wx)
        self.budget = budget(self.cover)


@functools.lru_cache(maxsize=None)
def cases():
    """Every entry of CASES, drawn in order from ONE ``default_rng(0)``."""
    rng = np.random.default_rng(0)
    return [Case(spec, rng) for spec in CASES]
