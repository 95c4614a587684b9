// Dual-task consistency (DTC, Luo et al. 2021; reference network/dtc.py) after the two heads: the supervision target and the loss.
//   * dense batched 2-D distance transform: for every class c of every label slice b, with membership P = (label == c), the exact squared
//     Euclidean distance d2 from each pixel to the nearest pixel whose membership DIFFERS from its own (members: to the nearest
//     non-member; non-members: to the nearest member).  Outside the image is nothing.  d2 = 0 everywhere where P is empty or full.
//   * the normalised signed distance map sdf = +sqrt(d2 / max d2 over non-members) on non-members, -sqrt(d2 / max d2 over members) on
//     members, exactly 0 on the inner boundary (members with d2 == 1), exactly +1 where P is empty and -1 where P is full.
//   * the fused loss [mean (t[:B] - sdf)^2, mean (sigmoid(-k t) - softmax(z))^2] and its backward to t and z in one launch.
// One transform per image serves both signs, because every pixel needs only the distance to the OTHER set:
//   k_sdf_rows   one wave per 64 pixels of a label row: the row is read once for all classes, __ballot(label == c) is the membership
//                word of class c -> bits[b][c][y][W/64 words] (8 bytes per 64 pixels and class: 0.3 MB at 8 x 5 x 256^2).
//   k_sdf_cols   one workgroup per (image, 64-column tile).  Row pass: a pixel's distance along x to the nearest bit of the other set,
//                by __clzll / __ffsll over the row's words (no scan over pixels), as ONE signed 16-bit value per pixel in LDS:
//                +g on a member (g = distance to the nearest non-member of the row), -g on a non-member, +-GINF where the row has
//                none.  H x 64 shorts: 32 KB at H = 256, 64 KB at H = 512.  Column pass: d2 = min over y' of v(y')^2 + (y - y')^2 with
//                v(y') = max(s, 0) for a member, max(-s, 0) for a non-member; rows are visited outwards from y and a lane stops once
//                (y - y')^2 reaches its best.  A tile whose rows are all +GINF or all -GINF belongs to a full or empty image and writes
//                zeros without a search.  The two maxima per image go through integer atomicMax: exact and order-free.
//   k_sdf_final  sdf in NHWC (the layout of the tanh head it is compared with), one thread per pixel and all classes.
// Labels int64 [B][H][W]; a label outside [0, C) is a member of no class and raises the caller's status word (plain store of 1).
// Loss statistics: per-workgroup partials in double, summed by one workgroup in a fixed order: reproducible run to run.
#include "common.h"
#include <mutex>

namespace {
constexpr int TPB = 256;
constexpr int MAXC = 16;
constexpr int MAXHW = 512;
constexpr int GINF = 0x7FFF;                     // "no pixel of the other set in this row"; GINF^2 + 511^2 < 2^31
constexpr int GINF2 = GINF * GINF;
typedef unsigned long long u64;

__host__ __device__ inline int words_per_row(int W) { return (W + 63) >> 6; }

// ---- membership words.  grid (ceil(H * WPR / 4), B): wave = one (row, word)
__global__ void __launch_bounds__(TPB)
k_sdf_rows(const int64_t* __restrict__ labels, u64* __restrict__ bits, int* __restrict__ maxima, int* __restrict__ status, int C, int H,
           int W) {
  const int WPR = words_per_row(W);
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  if (blockIdx.x == 0 && threadIdx.x < 2 * C) maxima[b * 2 * C + threadIdx.x] = 0;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (item >= H * WPR) return;                                      // (wave-uniform)
  const int y = item / WPR, word = item - y * WPR;
  const int x = word * 64 + lane;
  long long lab = -1;
  if (x < W) {
    lab = labels[((size_t)b * H + y) * W + x];
    if (lab < 0 || lab >= C) { *status = 1; lab = -1; }
  }
  u64 mine = 0;
  for (int c = 0; c < C; ++c) {
    const u64 m = __ballot(lab == c);
    if (lane == c) mine = m;
  }
  if (lane < C) bits[(((size_t)b * C + lane) * H + y) * WPR + word] = mine;
}

// distance from bit position x to the nearest set bit of the row words m[0..WPR), GINF when there is none
__device__ __forceinline__ int nearest_bit(const u64 (&m)[8], int WPR, int x) {
  const int wi = x >> 6, bp = x & 63;
  int best = GINF;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j < WPR) {                                                  // (uniform)
      const u64 w = m[j];
      if (j < wi) {
        if (w) best = min(best, x - (j * 64 + 63 - __clzll((long long)w)));
      } else if (j > wi) {
        if (w) best = min(best, j * 64 + __ffsll((long long)w) - 1 - x);
      } else {
        const u64 lo = w & (((u64)2 << bp) - 1);                    // bits <= bp  ((2 << 63) wraps to 0: all bits)
        const u64 hi = w >> bp;                                     // bits >= bp
        if (lo) best = min(best, bp - (63 - __clzll((long long)lo)));
        if (hi) best = min(best, __ffsll((long long)hi) - 1);
      }
    }
  }
  return best;
}

// ---- grid (WPR, B * C), dynamic LDS = H * 64 shorts
__global__ void __launch_bounds__(TPB)
k_sdf_cols(const u64* __restrict__ bits, int* __restrict__ d2, int* __restrict__ maxima, int H, int W) {
  extern __shared__ short g[];                                      // [H][64]
  const int WPR = words_per_row(W);
  const int tile = blockIdx.x, img = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x = tile * 64 + lane;
  const u64* ib = bits + (size_t)img * H * WPR;
  // row pass
  bool all_pos = true, all_neg = true;                              // every pixel of the tile: member / non-member of a row without the other set
  for (int y = wave; y < H; y += 4) {
    u64 mem[8], non[8], own = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int nb = W - j * 64;                                    // bits of word j inside the image
      const u64 valid = nb >= 64 ? ~(u64)0 : (nb > 0 ? ((u64)1 << nb) - 1 : 0);
      const u64 w = j < WPR ? ib[(size_t)y * WPR + j] : 0;
      mem[j] = w;
      non[j] = ~w & valid;
      own = j == tile ? w : own;                                    // (register select: no dynamic index into mem)
    }
    const bool member = (own >> lane) & 1;
    const int s = member ? nearest_bit(non, WPR, x) : -nearest_bit(mem, WPR, x);
    g[y * 64 + lane] = (short)s;
    if (x < W) { all_pos = all_pos && s == GINF; all_neg = all_neg && s == -GINF; }
  }
  int* out = d2 + (size_t)img * H * W;
  // every row of the tile's columns is all members, or every row all non-members (a row is one or the other across its whole width when
  // its value is +-GINF): the image has no pixel of the other set -- P is full or empty, d2 = 0, the maxima stay 0.  Without this exit
  // every lane would walk its whole column (an absent class; a background-only slice gives C such images).
  const int full = __syncthreads_and(all_pos), empty = __syncthreads_and(all_neg);       // (also the barrier after the row pass)
  if (full || empty) {
    for (int y = wave; y < H; y += 4)
      if (x < W) out[(size_t)y * W + x] = 0;
    return;
  }
  // column pass
  int mx_mem = 0, mx_non = 0;
  for (int y = wave; y < H; y += 4) {
    const int s = g[y * 64 + lane];
    const bool member = s > 0;
    const int v0 = member ? s : -s;
    int best = v0 * v0;
    for (int dy = 1; dy < H; ++dy) {                                // (the trip count is the wave's slowest lane's)
      const int dd = dy * dy;
      if (__all(dd >= best)) break;
      if (dd < best) {
        if (y - dy >= 0) {
          const int t = g[(y - dy) * 64 + lane];
          const int v = member ? max(t, 0) : max(-t, 0);
          best = min(best, v * v + dd);
        }
        if (y + dy < H) {
          const int t = g[(y + dy) * 64 + lane];
          const int v = member ? max(t, 0) : max(-t, 0);
          best = min(best, v * v + dd);
        }
      }
    }
    if (best >= GINF2) best = 0;                                    // the other set is empty: P is empty or full
    if (x < W) {
      out[(size_t)y * W + x] = best;
      if (member) mx_mem = max(mx_mem, best); else mx_non = max(mx_non, best);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx_mem = max(mx_mem, __shfl_xor(mx_mem, o, 64));
    mx_non = max(mx_non, __shfl_xor(mx_non, o, 64));
  }
  if (lane == 0) {
    if (mx_non) atomicMax(maxima + img * 2, mx_non);
    if (mx_mem) atomicMax(maxima + img * 2 + 1, mx_mem);
  }
}

// ---- sdf[b][p][c] (NHWC) from d2[b][c][p]; maxima[b][c] = {max over non-members, max over members}
__global__ void __launch_bounds__(TPB)
k_sdf_final(const int64_t* __restrict__ labels, const int* __restrict__ d2, const int* __restrict__ maxima, float* __restrict__ sdf, int B,
            int C, int HW) {
  const int64_t P = (int64_t)B * HW;
  for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < P; i += (int64_t)gridDim.x * TPB) {
    const int b = (int)(i / HW);
    const int p = (int)(i - (int64_t)b * HW);
    const long long lab = labels[i];
    for (int c = 0; c < C; ++c) {
      const int d = d2[((size_t)b * C + c) * HW + p];
      const bool member = lab == c;
      float v;
      if (d == 0) v = member ? -1.f : 1.f;                          // P empty (+1 everywhere) or full (-1 everywhere)
      else if (member) v = d == 1 ? 0.f : -(float)sqrt((double)d / (double)maxima[(b * C + c) * 2 + 1]);
      else v = (float)sqrt((double)d / (double)maxima[(b * C + c) * 2]);
      sdf[i * C + c] = v;
    }
  }
}

// ---- the loss.  CT > 0: C as a compile-time constant; CT = 0: runtime C <= MAXC, loops unrolled to MAXC with the channels past C
// loaded as -inf logits (probability exactly 0) and skipped in the sums, so the per-channel arrays stay in registers (k_dicece_partial).
template <int CT>
struct Px {
  static constexpr int CC = CT ? CT : MAXC;
  float t[CC], p[CC], s[CC], a[CC];             // tanh head, softmax(z), sigmoid(-k t), exp(-|k t|)

  __device__ __forceinline__ void load(const float* __restrict__ tp, const float* __restrict__ zp, int C, float k) {
    float z[CC], m = -INFINITY;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      const bool on = CT || c < C;
      t[c] = on ? tp[c] : 0.f;
      z[c] = on ? zp[c] : -INFINITY;
      m = fmaxf(m, z[c]);
    }
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CC; ++c) { p[c] = __expf(z[c] - m); sum += p[c]; }
    const float inv = 1.f / sum;
#pragma unroll
    for (int c = 0; c < CC; ++c) {
      p[c] *= inv;
      // sigmoid(x), x = -k t, from e = exp(-|x|) in (0, 1]: no overflow at |x| = 1500 (e = 0: exactly 0 or 1)
      const float xx = -k * t[c];
      const float e = expf(-fabsf(xx));
      a[c] = e;
      s[c] = (xx >= 0.f ? 1.f : e) / (1.f + e);
    }
  }
};

// part[blk] = {sum (t - sdf)^2 (slices < B), sum (sigmoid(-k t) - softmax(z))^2} in double.  grid (pb, N)
template <int CT>
__global__ void __launch_bounds__(TPB)
k_dtc_partial(const float* __restrict__ t, const float* __restrict__ z, const float* __restrict__ sdf, double* __restrict__ part, int B,
              int64_t HW, int Crt, float k) {
  constexpr int CC = Px<CT>::CC;
  const int C = CT ? CT : Crt;
  __shared__ double sm4[4];
  const int n = blockIdx.y;
  const bool lab = n < B;                                           // (uniform)
  float a0 = 0.f, a1 = 0.f;
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < HW; p += (int64_t)gridDim.x * TPB) {
    const int64_t off = ((int64_t)n * HW + p) * C;
    Px<CT> q;
    q.load(t + off, z + off, C, k);
#pragma unroll
    for (int c = 0; c < CC; ++c)
      if (CT || c < C) {
        const float d = q.s[c] - q.p[c];
        a1 += d * d;
        if (lab) { const float e = q.t[c] - sdf[off + c]; a0 += e * e; }
      }
  }
  const double s0 = block_sum_256_d((double)a0, sm4);
  const double s1 = block_sum_256_d((double)a1, sm4);
  if (threadIdx.x == 0) {
    const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    part[blk * 2] = s0;
    part[blk * 2 + 1] = s1;
  }
}

// out = [sum0 / m0, sum1 / m1]: one workgroup, fixed order
__global__ void __launch_bounds__(TPB)
k_dtc_final(const double* __restrict__ part, int nblk, double m0, double m1, float* __restrict__ out) {
  __shared__ double sm4[4];
  double a0 = 0.0, a1 = 0.0;
  for (int i = threadIdx.x; i < nblk; i += TPB) { a0 += part[(size_t)i * 2]; a1 += part[(size_t)i * 2 + 1]; }
  a0 = block_sum_256_d(a0, sm4);
  a1 = block_sum_256_d(a1, sm4);
  if (threadIdx.x == 0) { out[0] = (float)(a0 / m0); out[1] = (float)(a1 / m1); }
}

// gt = gout[0] d L_sdf / dt + gout[1] d L_cons / dt, gz = gout[1] d L_cons / dz.  With d_c = s_c - p_c:
//   d L_cons / dt_c = (2 / m1) d_c (-k) s_c (1 - s_c),   d L_cons / dz_j = (2 / m1) p_j (sum_c p_c d_c - d_j),   s (1 - s) = e / (1 + e)^2
template <int CT>
__global__ void __launch_bounds__(TPB)
k_dtc_bwd(const float* __restrict__ t, const float* __restrict__ z, const float* __restrict__ sdf, const float* __restrict__ gout,
          float* __restrict__ gt, float* __restrict__ gz, int B, int64_t HW, int Crt, float k, float w0, float w1) {
  constexpr int CC = Px<CT>::CC;
  const int C = CT ? CT : Crt;
  const int n = blockIdx.y;
  const bool lab = n < B;
  const float g0 = gout[0] * w0, g1 = gout[1] * w1;                 // w = 2 / m
  for (int64_t p = (int64_t)blockIdx.x * TPB + threadIdx.x; p < HW; p += (int64_t)gridDim.x * TPB) {
    const int64_t off = ((int64_t)n * HW + p) * C;
    Px<CT> q;
    q.load(t + off, z + off, C, k);
    float d[CC], dot = 0.f;
#pragma unroll
    for (int c = 0; c < CC; ++c) { d[c] = (CT || c < C) ? q.s[c] - q.p[c] : 0.f; dot += q.p[c] * d[c]; }
#pragma unroll
    for (int c = 0; c < CC; ++c)
      if (CT || c < C) {
        const float e1 = 1.f + q.a[c];
        float v = g1 * d[c] * (-k) * (q.a[c] / (e1 * e1));
        if (lab) v += g0 * (q.t[c] - sdf[off + c]);
        gt[off + c] = v;
        gz[off + c] = g1 * q.p[c] * (dot - d[c]);
      }
  }
}

// workgroups per slice: two pixels per thread at 256 x 256, at most 128 (cora_blocks of coranet.hip)
inline int dtc_blocks(int64_t HW) {
  int64_t b = cdiv64(HW, TPB * 2);
  if (b > 128) b = 128;
  if (b < 1) b = 1;
  return (int)b;
}
inline bool sdf_args_ok(int B, int C, int H, int W) {
  return B >= 1 && C >= 1 && C <= MAXC && H >= 1 && H <= MAXHW && W >= 1 && W <= MAXHW && (int64_t)B * C <= 65535;
}

}  // namespace

extern "C" {
#define ST ((hipStream_t)stream)
#define DTC_C(K, ...)                                          \
  switch (C) {                                                 \
    case 1: K<1> __VA_ARGS__; break;                           \
    case 2: K<2> __VA_ARGS__; break;                           \
    case 5: K<5> __VA_ARGS__; break;                           \
    default: K<0> __VA_ARGS__;                                 \
  }

// workspace floats of smsut_edt_sq: the two maxima per image (int), then the membership words (8 bytes each).  -1: unsupported shape.
int64_t smsut_sdf_ws(int B, int C, int H, int W) {
  if (!sdf_args_ok(B, C, H, W)) return -1;
  return 2 * (int64_t)B * C + 2 * (int64_t)B * C * H * words_per_row(W);
}

// d2[B][C][H][W] (int32): exact squared distance to the nearest pixel of the other set of class c's membership image; the workspace
// keeps {max over non-members, max over members} per image for smsut_sdf_final.  status: one device int, set to 1 by a label outside
// [0, C) (never cleared here).  1 <= H, W <= 512, 1 <= C <= 16.
int smsut_edt_sq(const int64_t* labels, int* d2, float* workspace, int* status, int B, int C, int H, int W, void* stream) {
  SMSUT_REQUIRE(labels && d2 && workspace && status && sdf_args_ok(B, C, H, W));
  const int WPR = words_per_row(W);
  int* maxima = (int*)workspace;
  u64* bits = (u64*)(maxima + 2 * (size_t)B * C);
  k_sdf_rows<<<dim3((unsigned)cdiv64((int64_t)H * WPR, 4), B), TPB, 0, ST>>>(labels, bits, maxima, status, C, H, W);
  // (up to 64 KB of dynamic LDS next to the 256 static bytes of the workgroup vote: past the 64 KB a launch gets without the attribute)
  static std::once_flag once;
  std::call_once(once, [] { (void)hipFuncSetAttribute((const void*)k_sdf_cols, hipFuncAttributeMaxDynamicSharedMemorySize, MAXHW * 64 * 2); });
  k_sdf_cols<<<dim3(WPR, B * C), TPB, (size_t)H * 64 * sizeof(short), ST>>>(bits, d2, maxima, H, W);
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}
// sdf[B][H][W][C] (fp32, NHWC) from d2 and the workspace smsut_edt_sq left
int smsut_sdf_final(const int64_t* labels, const int* d2, const float* workspace, float* sdf, int B, int C, int H, int W, void* stream) {
  SMSUT_REQUIRE(labels && d2 && workspace && sdf && sdf_args_ok(B, C, H, W));
  k_sdf_final<<<ew_grid((int64_t)B * H * W), TPB, 0, ST>>>(labels, d2, (const int*)workspace, sdf, B, C, H * W);
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

// workspace floats of smsut_dtc_loss_fwd (two doubles per workgroup)
int64_t smsut_dtc_ws(int N, int64_t HW) { return 4 * (int64_t)N * dtc_blocks(HW); }

// out[2] = [mean over B C HW of (t[:B] - sdf)^2, mean over N C HW of (sigmoid(-k t) - softmax(z)_c)^2]; t, z [N][HW][C], sdf [B][HW][C]
int smsut_dtc_loss_fwd(const float* t, const float* z, const float* sdf, float* out, void* workspace, int N, int B, int64_t HW, int C,
                       float k, void* stream) {
  SMSUT_REQUIRE(t && z && sdf && out && workspace && N > 0 && B >= 1 && B <= N && HW > 0 && C >= 1 && C <= MAXC);
  const int pb = dtc_blocks(HW);
  double* part = (double*)workspace;
  DTC_C(k_dtc_partial, <<<dim3(pb, N), TPB, 0, ST>>>(t, z, sdf, part, B, HW, C, k));
  k_dtc_final<<<1, TPB, 0, ST>>>(part, N * pb, (double)B * (double)C * (double)HW, (double)N * (double)C * (double)HW, out);
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}
// gt, gz [N][HW][C] from gout[2] = [d / d L_sdf, d / d L_cons]; sdf gets no gradient
int smsut_dtc_loss_bwd(const float* t, const float* z, const float* sdf, const float* gout, float* gt, float* gz, int N, int B, int64_t HW,
                       int C, float k, void* stream) {
  SMSUT_REQUIRE(t && z && sdf && gout && gt && gz && N > 0 && B >= 1 && B <= N && HW > 0 && C >= 1 && C <= MAXC);
  const float w0 = (float)(2.0 / ((double)B * (double)C * (double)HW)), w1 = (float)(2.0 / ((double)N * (double)C * (double)HW));
  DTC_C(k_dtc_bwd, <<<dim3(dtc_blocks(HW), N), TPB, 0, ST>>>(t, z, sdf, gout, gt, gz, B, HW, C, k, w0, w1));
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

}  // extern "C"
