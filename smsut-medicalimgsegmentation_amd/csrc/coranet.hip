// CoraNet (reference trainer/coraNetTrainer.py) after the logits, as streaming kernels over the 3L+1 output channels of the stock U-Net.
// The channels are three (L+1)-class heads that share the background logit: channel 0 is the background of every head, head k owns
// channels 1+kL .. (k+1)L.  The reference materialises each head with torch.cat and runs a separate loss on each; here every pass reads a
// pixel's 3L+1 logits once, does the three small softmaxes from the same registers, and (backward) writes the 3L+1 gradients once, the
// background channel receiving the sum of the three heads' contributions.
//   * supervised head loss (:288-301): S = ([w_dc Dice_batch(h0,y) + w_ce CE(h0,y)] + CE_wcon(h1,y) + CE_wrad(h2,y)) / 4
//   * pseudo-labelled head loss (:304-347): certain = (masked CE(h0,q) + Dice_per_sample(h0,q)) / 2,
//     uncertain = cw/3 * sum_k masked softmax-MSE(h_k(z), h_k(e)) with the mask inverted, denominators counting pixels
//   * pseudo labels q = argmax(h0), certainty mask m = (argmax(h1) == argmax(h2))  (:189-208)
//   * EMA over many tensors in one launch (:168-174)
// Logits NHWC [N][HW][3L+1] fp32, labels int64 [N][HW], mask fp32 [N][HW].  Statistics: block partials (fp32), then a fixed-order fp64
// tree per statistic, so results are reproducible run to run.  The pixel stride is (3L+1)*4 bytes (52 at L = 4), never 16-byte aligned:
// the kernels keep per-lane dword loads as k_dicece_partial (loss.hip) does; a wave's 64 pixels are one contiguous span, so the 3L+1 loads
// of a wave together use every byte of the lines they touch.
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int MAXL = 10;                      // 3L+1 <= 32 channels (MAXC of loss.hip)
constexpr int MAXS = 3 * (MAXL + 1) + 4;      // statistics per group: {tp, sum_p, count} per class of head 0, then up to 4 scalars

// LT > 0: L as a compile-time constant.  LT = 0: runtime L <= MAXL -- the loops still unroll to MAXL with the classes past L loaded
// as -inf (probability exactly 0), so the per-class arrays stay in registers in this form too (runtime loop bounds index them
// dynamically and send them to scratch: the finding written at k_dicece_partial).
template <int LT>
struct Heads {
  static constexpr int LL = LT ? LT : MAXL;
  float z0;               // the shared background logit
  float z[3][LL];         // foreground logits per head
  float p0[3];            // background probability per head
  float p[3][LL];         // foreground probabilities per head
  float lse[3];           // log-sum-exp per head

  __device__ __forceinline__ void load(const float* __restrict__ px, int L) {
    z0 = px[0];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < LL; ++j) z[k][j] = (LT || j < L) ? px[1 + k * L + j] : -INFINITY;
  }
  __device__ __forceinline__ void softmax() {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float m = z0;
#pragma unroll
      for (int j = 0; j < LL; ++j) m = fmaxf(m, z[k][j]);
      const float e0 = __expf(z0 - m);
      float s = e0;
#pragma unroll
      for (int j = 0; j < LL; ++j) { p[k][j] = __expf(z[k][j] - m); s += p[k][j]; }
      const float inv = 1.f / s;
      p0[k] = e0 * inv;
#pragma unroll
      for (int j = 0; j < LL; ++j) p[k][j] *= inv;
      lse[k] = m + __logf(s);
    }
  }
  // the logit of class `lab` in head k (register select, no dynamic indexing)
  __device__ __forceinline__ float at(int k, int lab) const {
    float v = z0;
#pragma unroll
    for (int j = 0; j < LL; ++j) v = lab == j + 1 ? z[k][j] : v;
    return v;
  }
  // first maximum of head k, as torch.argmax (NaN wins)
  __device__ __forceinline__ int argmax(int k) const {
    float best = z0;
    int bi = 0;
#pragma unroll
    for (int j = 0; j < LL; ++j) {
      const float v = z[k][j];
      if (v > best || (v != v && best == best)) { best = v; bi = j + 1; }     // (a class past L is -inf: never greater)
    }
    return bi;
  }
};

// per-class {tp, sum_p, count} of head 0 against `lab`, the Dice statistics of loss.hip
template <int LT>
__device__ __forceinline__ void dice_acc(const Heads<LT>& h, int lab, float (&tp)[Heads<LT>::LL + 1], float (&sp)[Heads<LT>::LL + 1],
                                         float (&cnt)[Heads<LT>::LL + 1]) {
  sp[0] += h.p0[0];
  if (lab == 0) { tp[0] += h.p0[0]; cnt[0] += 1.f; }
#pragma unroll
  for (int j = 0; j < Heads<LT>::LL; ++j) {
    sp[j + 1] += h.p[0][j];
    if (lab == j + 1) { tp[j + 1] += h.p[0][j]; cnt[j + 1] += 1.f; }
  }
}

// wave sums -> red[4][MAXS] (one row per wave); after the barrier the first `ns` threads add the four rows
#define CORA_PUT(idx, val)                                    \
  do {                                                        \
    const float v__ = wave_sum(val);                          \
    if (lane == 0) red[wave * MAXS + (idx)] = v__;            \
  } while (0)

template <int LT>
__device__ __forceinline__ void dice_put(const float (&tp)[Heads<LT>::LL + 1], const float (&sp)[Heads<LT>::LL + 1],
                                         const float (&cnt)[Heads<LT>::LL + 1], int L, float* red, int lane, int wave) {
#pragma unroll
  for (int c = 0; c <= Heads<LT>::LL; ++c)
    if (LT || c <= L) {                                       // (uniform)
      CORA_PUT(c * 3, tp[c]);
      CORA_PUT(c * 3 + 1, sp[c]);
      CORA_PUT(c * 3 + 2, cnt[c]);
    }
}

// ---- supervised head loss, stage 1.  part[blk][3(L+1)+3] = head-0 Dice statistics, sum nll(h0), sum w_con[y] nll(h1), sum w_rad[y] nll(h2)
// (the weighted-CE denominators sum_p w[y_p] follow from the class counts: sum_c w[c] count[c])
template <int LT>
__global__ void __launch_bounds__(TPB)
k_cora_sup_partial(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ w_con,
                   const float* __restrict__ w_rad, float* __restrict__ part, int64_t HW, int Lrt) {
  constexpr int LL = Heads<LT>::LL;
  const int L = LT ? LT : Lrt;
  const int C = 3 * L + 1, NS = 3 * (L + 1) + 3;
  __shared__ float red[4 * MAXS];
  __shared__ float wsm[2][MAXL + 1];
  if (threadIdx.x <= L) { wsm[0][threadIdx.x] = w_con[threadIdx.x]; wsm[1][threadIdx.x] = w_rad[threadIdx.x]; }
  __syncthreads();
  const int n = blockIdx.y;
  float tp[LL + 1], sp[LL + 1], cnt[LL + 1];
#pragma unroll
  for (int c = 0; c <= LL; ++c) { tp[c] = 0.f; sp[c] = 0.f; cnt[c] = 0.f; }
  float ce0 = 0.f, wn1 = 0.f, wn2 = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < HW; p += (int64_t)gridDim.x * TPB) {
    const int64_t pix = (int64_t)n * HW + p;
    const int lab = (int)labels[pix];
    Heads<LT> h;
    h.load(logits + pix * C, L);
    h.softmax();
    dice_acc<LT>(h, lab, tp, sp, cnt);
    if (lab >= 0 && lab <= L) {
      ce0 += h.lse[0] - h.at(0, lab);
      wn1 += wsm[0][lab] * (h.lse[1] - h.at(1, lab));
      wn2 += wsm[1][lab] * (h.lse[2] - h.at(2, lab));
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  dice_put<LT>(tp, sp, cnt, L, red, lane, wave);
  CORA_PUT(3 * (L + 1), ce0);
  CORA_PUT(3 * (L + 1) + 1, wn1);
  CORA_PUT(3 * (L + 1) + 2, wn2);
  __syncthreads();
  const int blk = blockIdx.y * gridDim.x + blockIdx.x;
  if (threadIdx.x < NS)
    part[(size_t)blk * NS + threadIdx.x] = red[threadIdx.x] + red[MAXS + threadIdx.x] + red[2 * MAXS + threadIdx.x] + red[3 * MAXS + threadIdx.x];
}

// stats[g][s] = sum over the nbg blocks of group g of part[blk][s]: one 256-thread block per output word, fp64 tree in a fixed order
__global__ void __launch_bounds__(TPB)
k_cora_reduce(const float* __restrict__ part, int nbg, int NS, float* __restrict__ stats) {
  __shared__ double sm4[4];
  const int s = blockIdx.x, g = blockIdx.y;
  double acc = 0.0;
  for (int b = threadIdx.x; b < nbg; b += TPB) acc += (double)part[((size_t)g * nbg + b) * NS + s];
  acc = block_sum_256_d(acc, sm4);
  if (threadIdx.x == 0) stats[(size_t)g * NS + s] = (float)acc;
}

__device__ __forceinline__ double dice_coeff(const float* s, float smooth, float eps) {
  // 2tp + fp + fn = sum_p + count (misc/loss.py:32-34,55-57)
  return (2.0 * (double)s[0] + (double)smooth) / ((double)s[1] + (double)s[2] + (double)smooth + (double)eps);
}

// out = [S, w_dc dice + w_ce ce of head 0, con, rad]
__global__ void k_cora_sup_final(const float* __restrict__ stats, const float* __restrict__ w_con, const float* __restrict__ w_rad, int L,
                                 double npix_total, float w_dc, float w_ce, float smooth, float eps, float* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  double acc = 0.0, dcon = 0.0, drad = 0.0;
  for (int c = 0; c <= L; ++c) {
    if (c) acc += dice_coeff(stats + c * 3, smooth, eps);
    dcon += (double)w_con[c] * (double)stats[c * 3 + 2];
    drad += (double)w_rad[c] * (double)stats[c * 3 + 2];
  }
  const float* sc = stats + 3 * (L + 1);
  const double dice = 1.0 - acc / (double)L;
  const double h0 = (double)w_dc * dice + (double)w_ce * ((double)sc[0] / npix_total);
  const double con = (double)sc[1] / dcon, rad = (double)sc[2] / drad;
  out[0] = (float)((h0 + con + rad) * 0.25);
  out[1] = (float)h0;
  out[2] = (float)con;
  out[3] = (float)rad;
}

// A[c], Bc[c]: dL/dp_c = Bc[c] - onehot * A[c] of a Dice term weighted k per foreground class (k_dicece_bwd, loss.hip)
__device__ __forceinline__ void dice_grad_coeff(const float* s, double k, float smooth, float eps, float& a, float& b) {
  const double den = (double)s[1] + (double)s[2] + (double)smooth + (double)eps;
  a = (float)(k * 2.0 / den);
  b = (float)(k * (2.0 * (double)s[0] + (double)smooth) / (den * den));
}

template <int LT>
__global__ void __launch_bounds__(TPB)
k_cora_sup_bwd(const float* __restrict__ logits, const int64_t* __restrict__ labels, const float* __restrict__ stats,
               const float* __restrict__ w_con, const float* __restrict__ w_rad, const float* __restrict__ gout,
               float* __restrict__ glogits, int64_t HW, int Lrt, double npix_total, float w_dc, float w_ce, float smooth, float eps) {
  constexpr int LL = Heads<LT>::LL;
  const int L = LT ? LT : Lrt;
  const int C = 3 * L + 1;
  __shared__ float A[MAXL + 1], Bc[MAXL + 1], wsm[2][MAXL + 1], invden[2];
  if (threadIdx.x <= L) {
    const int c = threadIdx.x;
    dice_grad_coeff(stats + c * 3, c == 0 ? 0.0 : (double)w_dc / (double)L, smooth, eps, A[c], Bc[c]);
    wsm[0][c] = w_con[c];
    wsm[1][c] = w_rad[c];
  }
  if (threadIdx.x == 64) {
    double dcon = 0.0, drad = 0.0;
    for (int c = 0; c <= L; ++c) {
      dcon += (double)w_con[c] * (double)stats[c * 3 + 2];
      drad += (double)w_rad[c] * (double)stats[c * 3 + 2];
    }
    invden[0] = (float)(1.0 / dcon);
    invden[1] = (float)(1.0 / drad);
  }
  __syncthreads();
  const int n = blockIdx.y;
  const float go = gout[0] * 0.25f;
  const float cew = (float)((double)w_ce / npix_total);
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < HW; p += (int64_t)gridDim.x * TPB) {
    const int64_t pix = (int64_t)n * HW + p;
    const int lab = (int)labels[pix];
    Heads<LT> h;
    h.load(logits + pix * C, L);
    h.softmax();
    float* gz = glogits + pix * C;
    const bool valid = lab >= 0 && lab <= L;
    // head 0: Dice through the softmax + CE
    float dp0 = Bc[0] - (lab == 0 ? A[0] : 0.f), dp[LL];
    float dot = h.p0[0] * dp0;
#pragma unroll
    for (int j = 0; j < LL; ++j) {
      dp[j] = (LT || j < L) ? Bc[j + 1] - (lab == j + 1 ? A[j + 1] : 0.f) : 0.f;
      dot += h.p[0][j] * dp[j];
    }
    const float c0 = valid ? cew : 0.f;
    float g0 = h.p0[0] * (dp0 - dot) + c0 * (h.p0[0] - (lab == 0 ? 1.f : 0.f));
#pragma unroll
    for (int j = 0; j < LL; ++j)
      if (LT || j < L) gz[1 + j] = go * (h.p[0][j] * (dp[j] - dot) + c0 * (h.p[0][j] - (lab == j + 1 ? 1.f : 0.f)));
    // heads 1, 2: class-weighted CE
#pragma unroll
    for (int k = 1; k < 3; ++k) {
      const float f = valid ? wsm[k - 1][lab] * invden[k - 1] : 0.f;
      g0 += f * (h.p0[k] - (lab == 0 ? 1.f : 0.f));
#pragma unroll
      for (int j = 0; j < LL; ++j)
        if (LT || j < L) gz[1 + k * L + j] = go * f * (h.p[k][j] - (lab == j + 1 ? 1.f : 0.f));
    }
    gz[0] = go * g0;
  }
}

// ---- pseudo-labelled head loss, stage 1.  part[blk][3(L+1)+4] per sample: head-0 Dice statistics against q, then
// sum m nll(h0, q), sum m, sum (1-m) sum_k sum_c (softmax(h_k(z))_c - softmax(h_k(e))_c)^2, sum (1-m)
template <int LT>
__global__ void __launch_bounds__(TPB)
k_cora_semi_partial(const float* __restrict__ z, const float* __restrict__ e, const int64_t* __restrict__ q, const float* __restrict__ m,
                    float* __restrict__ part, int64_t HW, int Lrt) {
  constexpr int LL = Heads<LT>::LL;
  const int L = LT ? LT : Lrt;
  const int C = 3 * L + 1, NS = 3 * (L + 1) + 4;
  __shared__ float red[4 * MAXS];
  const int n = blockIdx.y;
  float tp[LL + 1], sp[LL + 1], cnt[LL + 1];
#pragma unroll
  for (int c = 0; c <= LL; ++c) { tp[c] = 0.f; sp[c] = 0.f; cnt[c] = 0.f; }
  float mnll = 0.f, msum = 0.f, umse = 0.f, usum = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < HW; p += (int64_t)gridDim.x * TPB) {
    const int64_t pix = (int64_t)n * HW + p;
    const int lab = (int)q[pix];
    const float mk = m[pix];
    Heads<LT> hz, he;
    hz.load(z + pix * C, L);
    he.load(e + pix * C, L);
    hz.softmax();
    he.softmax();
    dice_acc<LT>(hz, lab, tp, sp, cnt);
    if (lab >= 0 && lab <= L) mnll += mk * (hz.lse[0] - hz.at(0, lab));
    msum += mk;
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float d0 = hz.p0[k] - he.p0[k];
      d2 += d0 * d0;
#pragma unroll
      for (int j = 0; j < LL; ++j) { const float d = hz.p[k][j] - he.p[k][j]; d2 += d * d; }
    }
    umse += (1.f - mk) * d2;
    usum += 1.f - mk;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  dice_put<LT>(tp, sp, cnt, L, red, lane, wave);
  CORA_PUT(3 * (L + 1), mnll);
  CORA_PUT(3 * (L + 1) + 1, msum);
  CORA_PUT(3 * (L + 1) + 2, umse);
  CORA_PUT(3 * (L + 1) + 3, usum);
  __syncthreads();
  const int blk = blockIdx.y * gridDim.x + blockIdx.x;
  if (threadIdx.x < NS)
    part[(size_t)blk * NS + threadIdx.x] = red[threadIdx.x] + red[MAXS + threadIdx.x] + red[2 * MAXS + threadIdx.x] + red[3 * MAXS + threadIdx.x];
}

// the four scalar sums over the samples, in sample order
__device__ __forceinline__ void semi_totals(const float* stats, int N, int L, double (&t)[4]) {
  const int NS = 3 * (L + 1) + 4;
  t[0] = t[1] = t[2] = t[3] = 0.0;
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < 4; ++i) t[i] += (double)stats[(size_t)n * NS + 3 * (L + 1) + i];
}

// out = [certain, uncertain]
__global__ void k_cora_semi_final(const float* __restrict__ stats, int N, int L, float cw, float smooth, float eps, float* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  const int NS = 3 * (L + 1) + 4;
  double acc = 0.0;
  for (int n = 0; n < N; ++n)
    for (int c = 1; c <= L; ++c) acc += dice_coeff(stats + (size_t)n * NS + c * 3, smooth, eps);
  const double dice = 1.0 - acc / ((double)N * (double)L);
  double t[4];
  semi_totals(stats, N, L, t);
  out[0] = (float)((t[0] / (t[1] + 1e-16) + dice) * 0.5);
  out[1] = (float)((double)cw / 3.0 * (t[2] / (t[3] + 1e-16)));
}

// gradient to z only (e is the EMA teacher); gout = [d/d certain, d/d uncertain]
template <int LT>
__global__ void __launch_bounds__(TPB)
k_cora_semi_bwd(const float* __restrict__ z, const float* __restrict__ e, const int64_t* __restrict__ q, const float* __restrict__ m,
                const float* __restrict__ stats, const float* __restrict__ gout, float* __restrict__ gz_all, int N, int64_t HW, int Lrt,
                float cw, float smooth, float eps) {
  constexpr int LL = Heads<LT>::LL;
  const int L = LT ? LT : Lrt;
  const int C = 3 * L + 1, NS = 3 * (L + 1) + 4;
  __shared__ float A[MAXL + 1], Bc[MAXL + 1], inv[2];
  const int n = blockIdx.y;
  if (threadIdx.x <= L) {
    const int c = threadIdx.x;
    dice_grad_coeff(stats + (size_t)n * NS + c * 3, c == 0 ? 0.0 : 1.0 / ((double)N * (double)L), smooth, eps, A[c], Bc[c]);
  }
  if (threadIdx.x == 64) {
    double t[4];
    semi_totals(stats, N, L, t);
    inv[0] = (float)(1.0 / (t[1] + 1e-16));
    inv[1] = (float)(1.0 / (t[3] + 1e-16));
  }
  __syncthreads();
  const float gc = gout[0] * 0.5f;
  const float gu = gout[1] * (cw * (2.f / 3.f)) * inv[1];
  const float gm = gc * inv[0];
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < HW; p += (int64_t)gridDim.x * TPB) {
    const int64_t pix = (int64_t)n * HW + p;
    const int lab = (int)q[pix];
    const float mk = m[pix];
    Heads<LT> hz, he;
    hz.load(z + pix * C, L);
    he.load(e + pix * C, L);
    hz.softmax();
    he.softmax();
    float* gz = gz_all + pix * C;
    // head 0: per-sample Dice + masked CE
    float dp0 = Bc[0] - (lab == 0 ? A[0] : 0.f), dp[LL];
    float dot = hz.p0[0] * dp0;
#pragma unroll
    for (int j = 0; j < LL; ++j) {
      dp[j] = (LT || j < L) ? Bc[j + 1] - (lab == j + 1 ? A[j + 1] : 0.f) : 0.f;
      dot += hz.p[0][j] * dp[j];
    }
    const float fm = (lab >= 0 && lab <= L) ? gm * mk : 0.f;
    float g0 = gc * hz.p0[0] * (dp0 - dot) + fm * (hz.p0[0] - (lab == 0 ? 1.f : 0.f));
    float gh0[LL];
#pragma unroll
    for (int j = 0; j < LL; ++j) gh0[j] = gc * hz.p[0][j] * (dp[j] - dot) + fm * (hz.p[0][j] - (lab == j + 1 ? 1.f : 0.f));
    // every head: masked softmax-MSE against the teacher
    const float fu = gu * (1.f - mk);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float d0 = hz.p0[k] - he.p0[k];
      float dk = hz.p0[k] * d0;
#pragma unroll
      for (int j = 0; j < LL; ++j) dk += hz.p[k][j] * (hz.p[k][j] - he.p[k][j]);
      g0 += fu * hz.p0[k] * (d0 - dk);
#pragma unroll
      for (int j = 0; j < LL; ++j)
        if (LT || j < L) {
          const float v = fu * hz.p[k][j] * ((hz.p[k][j] - he.p[k][j]) - dk);
          gz[1 + k * L + j] = k == 0 ? gh0[j] + v : v;
        }
    }
    gz[0] = g0;
  }
}

// q = argmax(h0) (int64), m = (argmax(h1) == argmax(h2)) (fp32 0/1); first maximum wins, so the background wins a tie
template <int LT>
__global__ void __launch_bounds__(TPB)
k_cora_pseudo(const float* __restrict__ z, int64_t* __restrict__ q, float* __restrict__ m, int64_t P, int Lrt) {
  const int L = LT ? LT : Lrt;
  const int C = 3 * L + 1;
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < P; p += (int64_t)gridDim.x * TPB) {
    Heads<LT> h;
    h.load(z + p * C, L);
    q[p] = h.argmax(0);
    m[p] = h.argmax(1) == h.argmax(2) ? 1.f : 0.f;
  }
}

// ---- EMA over MANY tensors in one launch: ema = alpha ema + (1 - alpha) p, with the entry / block tables of k_sgd_multi (pointwise.hip):
// one block per 8192-element chunk of one tensor
struct EmaEnt { float* ema; const float* p; long long n; };
constexpr int EMA_CHUNK = 8192;
__global__ void __launch_bounds__(TPB)
k_ema_multi(const EmaEnt* __restrict__ ents, const int* __restrict__ blk_ent, const int* __restrict__ blk_chunk, float alpha, float beta) {
  const EmaEnt t = ents[blk_ent[blockIdx.x]];
  const long long base = (long long)blk_chunk[blockIdx.x] * EMA_CHUNK;
  const long long end = base + EMA_CHUNK < t.n ? base + EMA_CHUNK : t.n;
  for (long long i = base + threadIdx.x; i < end; i += TPB) t.ema[i] = alpha * t.ema[i] + beta * t.p[i];
}

// blocks per sample: two pixels per thread at 256 x 256, at most 128 (1024 workgroups on 256 CUs at a batch of 8)
inline int cora_blocks(int64_t HW) {
  int64_t b = cdiv64(HW, TPB * 2);
  if (b > 128) b = 128;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace

extern "C" {
#define ST ((hipStream_t)stream)
#define CORA_L(K, ...)                                         \
  switch (L) {                                                 \
    case 1: K<1> __VA_ARGS__; break;                           \
    case 2: K<2> __VA_ARGS__; break;                           \
    case 4: K<4> __VA_ARGS__; break;                           \
    default: K<0> __VA_ARGS__;                                 \
  }

// workspace floats of either statistics pass: blocks * (3(L+1) + 4)
int64_t smsut_cora_ws(int N, int64_t HW, int L) { return (int64_t)N * cora_blocks(HW) * (3 * (L + 1) + 4); }

// Supervised head loss, stage 1: stats[3(L+1)+3] = head-0 {tp, sum_p, count}[L+1], sum nll(h0), sum w_con[y] nll(h1), sum w_rad[y] nll(h2).
// w_con, w_rad: device arrays of L+1 floats.  Under data parallelism the caller all-reduces stats between stage 1 and stage 2.
int smsut_cora_sup_stats(const float* logits, const int64_t* labels, const float* w_con, const float* w_rad, float* stats,
                         float* workspace, int N, int64_t HW, int L, void* stream) {
  SMSUT_REQUIRE(logits && labels && w_con && w_rad && stats && workspace && N > 0 && HW > 0 && L >= 1 && L <= MAXL);
  const int pb = cora_blocks(HW), NS = 3 * (L + 1) + 3;
  CORA_L(k_cora_sup_partial, <<<dim3(pb, N), TPB, 0, ST>>>(logits, labels, w_con, w_rad, workspace, HW, L));
  k_cora_reduce<<<dim3(NS, 1), TPB, 0, ST>>>(workspace, N * pb, NS, stats);
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}
// Stage 2: out[4] = [S, w_dc dice + w_ce ce of head 0, con, rad].  npix_total = (global) N*HW.
int smsut_cora_sup_final(const float* stats, const float* w_con, const float* w_rad, float* out, int L, double npix_total, float w_dc,
                         float w_ce, void* stream) {
  SMSUT_REQUIRE(stats && w_con && w_rad && out && L >= 1 && L <= MAXL && npix_total > 0);
  k_cora_sup_final<<<1, 64, 0, ST>>>(stats, w_con, w_rad, L, npix_total, w_dc, w_ce, 1e-5f, 1e-8f, out);
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}
// glogits[N][HW][3L+1] = gout[0] * dS/dlogits, from the (global) statistics
int smsut_cora_sup_bwd(const float* logits, const int64_t* labels, const float* stats, const float* w_con, const float* w_rad,
                       const float* gout, float* glogits, int N, int64_t HW, int L, double npix_total, float w_dc, float w_ce,
                       void* stream) {
  SMSUT_REQUIRE(logits && labels && stats && w_con && w_rad && gout && glogits && N > 0 && HW > 0 && L >= 1 && L <= MAXL &&
                npix_total > 0);
  CORA_L(k_cora_sup_bwd, <<<dim3(cora_blocks(HW), N), TPB, 0, ST>>>(logits, labels, stats, w_con, w_rad, gout, glogits, HW, L,
                                                                     npix_total, w_dc, w_ce, 1e-5f, 1e-8f));
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

// Pseudo-labelled head loss, stage 1: stats[N][3(L+1)+4] per sample = head-0 {tp, sum_p, count}[L+1] against q, then
// sum m nll(h0, q), sum m, sum (1-m) sum_k |softmax(h_k(z)) - softmax(h_k(e))|^2, sum (1-m).
int smsut_cora_semi_stats(const float* z, const float* e, const int64_t* q, const float* m, float* stats, float* workspace, int N,
                          int64_t HW, int L, void* stream) {
  SMSUT_REQUIRE(z && e && q && m && stats && workspace && N > 0 && HW > 0 && L >= 1 && L <= MAXL);
  const int pb = cora_blocks(HW), NS = 3 * (L + 1) + 4;
  CORA_L(k_cora_semi_partial, <<<dim3(pb, N), TPB, 0, ST>>>(z, e, q, m, workspace, HW, L));
  k_cora_reduce<<<dim3(NS, N), TPB, 0, ST>>>(workspace, pb, NS, stats);
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}
// Stage 2: out[2] = [certain, uncertain]
int smsut_cora_semi_final(const float* stats, float* out, int N, int L, float cw, void* stream) {
  SMSUT_REQUIRE(stats && out && N > 0 && L >= 1 && L <= MAXL);
  k_cora_semi_final<<<1, 64, 0, ST>>>(stats, N, L, cw, 1e-5f, 1e-8f, out);
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}
// gz[N][HW][3L+1] = gout[0] * d certain/dz + gout[1] * d uncertain/dz
int smsut_cora_semi_bwd(const float* z, const float* e, const int64_t* q, const float* m, const float* stats, const float* gout,
                        float* gz, int N, int64_t HW, int L, float cw, void* stream) {
  SMSUT_REQUIRE(z && e && q && m && stats && gout && gz && N > 0 && HW > 0 && L >= 1 && L <= MAXL);
  CORA_L(k_cora_semi_bwd, <<<dim3(cora_blocks(HW), N), TPB, 0, ST>>>(z, e, q, m, stats, gout, gz, N, HW, L, cw, 1e-5f, 1e-8f));
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

// q[P] = argmax(h0), m[P] = (argmax(h1) == argmax(h2)) from logits [P][3L+1]
int smsut_cora_pseudo(const float* z, int64_t* q, float* m, int64_t P, int L, void* stream) {
  SMSUT_REQUIRE(z && q && m && P > 0 && L >= 1 && L <= MAXL);
  CORA_L(k_cora_pseudo, <<<ew_grid(P), TPB, 0, ST>>>(z, q, m, P, L));
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

// ents: device array of {ema, p, n} (3 x 8 bytes each); blk_ent / blk_chunk as smsut_sgd_momentum_multi (chunk = smsut_ema_chunk()).
// ema = alpha * ema + beta * p; the caller passes beta = 1 - alpha.
int smsut_ema_multi(const void* ents, const int* blk_ent, const int* blk_chunk, int nblocks, float alpha, float beta, void* stream) {
  SMSUT_REQUIRE(ents && blk_ent && blk_chunk && nblocks > 0);
  k_ema_multi<<<nblocks, TPB, 0, ST>>>((const EmaEnt*)ents, blk_ent, blk_chunk, alpha, beta);
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}
int smsut_ema_chunk(void) { return EMA_CHUNK; }

}  // extern "C"
