"""References of the uncertainty-aware mean teacher (UA-MT), whose device side -- a fused loss head and a trainer -- is not in the tree
yet: an fp64 restatement of the loss head, the bound B_H on an fp32 kernel's entropy, the threshold
schedule, the case draw for GPU tests and the shared description of the scenario of tests/golden/uamt.npz (used by the generator and
the CPU test).  Test infrastructure only.

The arithmetic a device kernel is expected to state, per pixel, all fp32, in this order: member by member in list order
m = max_k u_t[k]; e_k = expf(u_t[k] - m); s = e_0 + e_1 + ... in channel order; acc_k += e_k / s; then mean_k = acc_k / (float)T
(the arithmetic of the test-time-augmentation merge, csrc/tta.hip); H = -sum_k mean_k * logf(mean_k + 1e-6f) in channel order;
mask = H < thr.  ``entropy_fp32`` below emulates exactly that in numpy.

Definitions (UA-MT, Yu et al. 2019; the 2-D form of SSL4MIS).  With u_t the teacher's T Monte-Carlo logit tensors, p = mean_t
softmax(u_t, channel):  H = -sum_c p_c log(p_c + 1e-6);  mask = H < thr;  dist = sum_c (softmax(z) - softmax(e))_c^2;
L = sum(mask * dist) / (2 * sum(mask) + 1e-16) (the published constant 2, not the class count);  kept = mean(mask);  meanH = mean(H).

B_H, the bound on |H_kernel - H_fp64| for a GPU test.  eps = 2^-24 (half an ulp of fp32); the kernel's arithmetic is the one
stated above, with expf, logf and the division each within 1 ulp = 2 eps (the documented accuracy of the device library;
the division is correctly rounded in this build, 2 eps covers a build where it is not).  One member, one pixel, d_k = u_k - m <= 0,
q_k its exact softmax value:
  * fl(u_k - m) has relative error eps, so exp of it has relative error |d_k| eps; expf adds 2 eps: e_k is within (|d_k| + 2) eps;
  * s sums C positive terms in order: relative error at most sum_j q_j (|d_j| + 2) eps + (C - 1) eps <= (ln C + C + 1) eps, because
    |d_j| <= -ln q_j and sum_j q_j (-ln q_j) <= ln C;
  * the division adds 2 eps:  |delta q_k| <= eps q_k (-ln q_k) + K eps q_k  with  K = C + 5 + ln C.
The T quotients are added in order ((T - 1) eps on a positive sum) and divided by T (2 eps); -x ln x is concave, so the mean of
q_tk (-ln q_tk) over t is at most p_k (-ln p_k):  |delta p_k| <= eps p_k (-ln p_k + A)  with  A = K + T + 1.
f(p) = p log(p + 1e-6) has |f'(p)| <= 1 - ln p on (0, 1], so the error carried into H is at most
  eps sum_k p_k (A - ln p_k)(1 - ln p_k) = eps sum_k p_k (ln^2 p_k - (A + 1) ln p_k + A) <= eps (C 4 / e^2 + (A + 1) ln C + A)
(p ln^2 p <= 4 / e^2 on [0, 1]; sum_k p_k (-ln p_k) <= ln C; sum_k p_k = 1).  Evaluating H itself: fl(p + 1e-6f) moves the logarithm by
eps, logf by 2 eps |log|, the product by eps |log|: eps p_k (1 + 3 |ln p_k|) per term, eps (1 + 3 ln C) in all; the C terms, each of
magnitude at most 1 / e with sum H <= ln C, are added in order: (C - 1) eps ln C.  (1e-6f differs from 1e-6 by 2.5e-15: nothing.)
  B_H(C, T) = eps (4 C / e^2 + (A + 1) ln C + A + 1 + 3 ln C + (C - 1) ln C),   A = C + T + 6 + ln C
= 4.2e-6 at C = 5, T = 8, 6.4e-6 at C = 10, T = 3 and 2.4e-5 at the limits C = 32, T = 16; 5.7e-7 at C = 1, T = 1 (where the kernel's value is -logf(1 + 1e-6f), 4.6e-8 from
fp64's -log(1 + 1e-6))."""
import math

import numpy as np
import torch

from oracle import recipe

EPS32 = 2.0 ** -24


def entropy_bound(c, t):
    """B_H of the module docstring"""
    lc = math.log(c)
    a = c + t + 6 + lc
    return EPS32 * (4.0 * c / math.e ** 2 + (a + 1.0) * lc + a + 1.0 + 3.0 * lc + (c - 1.0) * lc)


def entropy_ref(members):
    """members [T, N, C, H, W] (any float dtype, or a list of [N, C, H, W]) -> fp64 H [N, H, W]"""
    if isinstance(members, (list, tuple)):
        members = torch.stack(list(members))
    p = torch.softmax(members.double(), dim=2).mean(dim=0)
    return -(p * torch.log(p + 1e-6)).sum(dim=1)


def loss_ref(z, e, members, thr, mask=None):
    """fp64 [L, kept, meanH] (differentiable in ``z``); ``mask`` [N, H, W] overrides ``H < thr`` (a GPU test passes the kernel's own
    mask, so that the loss and gradient comparison is free of mask flips).  Also returns the mask and H."""
    h = entropy_ref(members)
    if mask is None:
        mask = h < thr
    m = mask.double()
    dist = ((torch.softmax(z.double(), 1) - torch.softmax(e.double(), 1)) ** 2).sum(dim=1)
    loss = (m * dist).sum() / (2.0 * m.sum() + 1e-16)
    return torch.stack([loss, m.mean(), h.mean()]), mask, h


def entropy_fp32(members):
    """The kernel's stated arithmetic in numpy fp32, operation by operation (numpy's exp / log in place of the device's): fp32 H"""
    u = members.numpy().astype(np.float32)                            # [T, N, C, H, W]
    t, c = u.shape[0], u.shape[2]
    acc = np.zeros(u.shape[1:], dtype=np.float32)
    for i in range(t):
        ex = np.exp(u[i] - u[i].max(axis=1, keepdims=True))
        s = ex[:, 0].copy()
        for k in range(1, c):
            s = s + ex[:, k]
        acc = acc + ex / s[:, None]
    mean = acc / np.float32(t)
    term = mean * np.log(mean + np.float32(1e-6))
    h = term[:, 0].copy()
    for k in range(1, c):
        h = h + term[:, k]
    assert h.dtype == np.float32
    return -h


def rampup(cur, length):
    ph = 1.0 - np.clip(cur, 0.0, length) / length
    return float(np.exp(-5.0 * ph * ph))


def threshold(it, max_it, threshold_max=math.log(2)):
    """the published schedule: (0.75 + 0.25 * sigmoid_rampup(iter, max_iterations)) * ln 2"""
    return (0.75 + 0.25 * rampup(it, max_it)) * threshold_max


# ------------------------------------------------------------------------------------------- case builders
CASES = [(1, 2, 1, 1, 1), (2, 5, 24, 40, 8), (3, 4, 37, 50, 4), (2, 3, 64, 64, 2), (1, 10, 8, 8, 3), (1, 5, 16, 16, 16),
         (2, 5, 256, 256, 8), (2, 1, 9, 7, 3), (1, 3, 16, 32, 2), (1, 3, 19, 27, 2)]
# (N, C, H, W, T): one pixel and one member; odd pixel counts; a runtime class count (10); T = 16; many workgroups; one class
# (H = -log(1 + 1e-6), every pixel kept, L = 0); 512 and 513 pixels (a full 256-thread workgroup at two pixels per thread, and one past it).
THRESHOLDS = (0.75 * math.log(2), math.log(2))


def case(n, c, h, w, t):
    """(z, e, members [T, N, C, H, W]) fp32 CPU tensors (logical NCHW).  Independent random members would give entropies near ln C
    and an empty mask; here a shared per-pixel logit vector of random sharpness plus unit member noise spreads H over [0, ln C]."""
    rs = np.random.RandomState(7 + c + t)
    u = 3.0 * rs.standard_normal((1, n, h, w, c)) * rs.uniform(0.0, 1.5, (1, n, h, w, 1)) + rs.standard_normal((t, n, h, w, c))
    z = 2.0 * rs.standard_normal((n, h, w, c))
    e = 2.0 * rs.standard_normal((n, h, w, c))
    f = lambda a, perm: torch.from_numpy(a.astype(np.float32)).permute(*perm).contiguous()
    return f(z, (0, 3, 1, 2)), f(e, (0, 3, 1, 2)), f(u, (0, 1, 4, 2, 3))


# ------------------------------------------------------------------------------------------- the scenario of tests/golden/uamt.npz
C, WIDTH, SIZE, BS, EPOCH, IT0 = 5, 8, 32, 2, 20, 300
SEED_NET, SEED_EMA, STEP_SEEDS = 501, 502, (510, 520)
LR, MOMENTUM, WD, MAX_IT = 1e-2, 0.9, 1e-3, 200 * 150
LAMBDA_SEMI, EMA_DECAY, RAMPUP = 1.0, 0.99, 30
MC_SAMPLES, MC_CHUNK, NOISE_STD, NOISE_CLIP = 4, 2, 0.1, 0.2
POST = {"fc": "decoder.fc.weight", "l1": "decoder.layer1.conv2.weight", "pre": "encoder.pre_conv.weight"}
HEAD_CASES = ((1, 5, 8, 8, 3), (2, 3, 5, 7, 2))          # small head cases whose fp64 results the fixture records


def shapes():
    return recipe.unet_shapes(1, C, WIDTH)


def step_inputs(seed):
    """([labelled | unlabelled] images [2 BS, 1, S, S], labels [BS, S, S], target noise [BS, 1, S, S], Monte-Carlo noise
    [MC_SAMPLES * BS, 1, S, S]) of one step; the noises are clamp(randn * 0.1, -0.2, 0.2) from a seeded numpy stream"""
    img = recipe.synth_images((2 * BS, 1, SIZE, SIZE), seed)
    msk = recipe.synth_labels(BS, SIZE, SIZE, C, seed + 1, block=8)
    rs = np.random.RandomState(seed + 2)
    draw = lambda k: torch.from_numpy(np.clip(rs.standard_normal((k, 1, SIZE, SIZE)) * NOISE_STD, -NOISE_CLIP, NOISE_CLIP)).float()
    return img, msk, draw(BS), draw(MC_SAMPLES * BS)
