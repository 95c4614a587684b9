// Calibration statistics of a batch of logits in one pass (misc/utils.py: CalibrationMeter, fit_temperature; ops.calibration_stats):
// the reliability table, negative log-likelihood, Brier score and the two derivatives of the NLL by the inverse temperature that a
// Newton fit of the temperature needs.  The arithmetic per pixel is stated in include/smsut_hip.h and restated in
// tests/calibration_ref.py; out is laid out as
//   out[3 b + {0, 1, 2}]           = bin b:   {pixels, sum of conf, correct pixels}
//   out[3 B + 4 k + {0, 1, 2, 3}]  = class k: {pixels, correct pixels, sum of nll, sum of brier}   (k = the TRUE class)
//   out[3 B + 4 K + {0, 1, 2, 3}]  = {g, h, skipped, nonfinite}
// and is ADDED to (fp64), never zeroed here.
//
// k_calibration: the P = N H W pixels are one flat run of C-float rows; a workgroup takes 256-pixel tiles, grid-strided, and stages a
//   tile's span through LDS with 16-byte loads from the 16-byte boundary below its start (k_eval_overlap's copy: the up to three
//   floats in front of and behind the span are never read; C > 32: the K leading floats of each long row are read in place).
//   Everything that can be an integer is one, and is summed with integer LDS atomics (order-free):
//     per bin    {pixels | correct << 32} in one 64-bit word, and sum of conf * 2^28 -- conf = 1 / s with s in [1, 32] is an fp32
//                value in [2^-5, 1], a multiple of 2^-28, so the product is an exact integer;
//     per class  {pixels | correct << 32};  skipped;  nonfinite.
//   The four float sums (nll and brier per true class, g, h) are fp64 from the pixel on: per-lane registers when the class count
//   is a compile-time constant, else the lanes of each class present in the wave are summed by a butterfly and added to the wave's
//   LDS row by its first lane; then a butterfly per wave and the four waves in order.  Each workgroup WRITES one partial vector
//   (integers as int64, float sums as fp64) to the workspace: no global atomics, no float atomics.
// k_calibration_finish: thread i (64 per workgroup) adds slot i of the partial vectors in workgroup order, 16 loads in flight at a
//   time, and adds the total to out[i].
// The grid is a function of P alone, so two calls on the same input give the same bits on any device.
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MAXK = SMSUT_CALIB_MAX_CLASSES;
constexpr int MAXB = SMSUT_CALIB_MAX_BINS;
constexpr int STAGE_MAXC = 32;     // rows of up to this many channels go through LDS; longer rows are read in place
constexpr int MAX_GRID = 256;      // partial vectors at most: the finishing launch reads them all (one workgroup per CU of an MI355X)
constexpr int FIN_TPB = 64;        // slots per workgroup of the finishing launch (at most 324 slots: 6 workgroups)
constexpr int FIN_UNR = 16;        // partial vectors loaded before the first is added
constexpr float CONF_SCALE = 268435456.f;                      // 2^28

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__host__ __device__ inline int calib_len(int K, int B) { return 3 * B + 4 * K + 4; }

inline int calib_grid(int64_t P) {
  const int64_t ntiles = cdiv64(P, TPB);
  return (int)(ntiles < MAX_GRID ? ntiles : MAX_GRID);
}

// KT > 0: the class count as a compile-time constant; KT = 0: a runtime K <= 32 under fully unrolled, guarded loops (static register
// indexing either way).
template <int KT, bool STAGED>
__global__ void __launch_bounds__(TPB)
k_calibration(const float* __restrict__ logits, const int64_t* __restrict__ labels, unsigned long long* __restrict__ part, int64_t P,
              int C, int K, int B, float beta) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (KT) K = KT;
  constexpr int KK = KT ? KT : MAXK;
  constexpr int KA = KT ? KT : 1;
  const int tile_floats = STAGED ? ((TPB * C + 8 + 3) & ~3) : 0;
  const int nints = 2 * B + K + 2;
  const int nflt = 2 * K + 2;
  unsigned long long* ints = (unsigned long long*)(smem + tile_floats);        // [B][2], [K], skipped, nonfinite
  double* wsum = (double*)(ints + nints);                                        // [WAVES][2 K + 2]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double* wrow = wsum + (size_t)wave * nflt;
  for (int i = threadIdx.x; i < nints; i += TPB) ints[i] = 0;
  for (int i = threadIdx.x; i < WAVES * nflt; i += TPB) wsum[i] = 0.0;
  __syncthreads();
  double an[KA], ab[KA], ag = 0.0, ah = 0.0;
#pragma unroll
  for (int k = 0; k < KA; ++k) { an[k] = 0.0; ab[k] = 0.0; }
  const float bf = (float)B;
  const int mis = (int)(((uintptr_t)logits >> 2) & 3);         // floats of `logits` past a 16-byte boundary
  const int64_t ntiles = (P + TPB - 1) / TPB;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {          // (uniform: barriers inside)
    const int64_t p0 = tile * TPB;
    const int npx = (int)(P - p0 < TPB ? P - p0 : TPB);
    const int64_t s0 = p0 * C;                                 // first float of the tile's span
    const bool valid = (int)threadIdx.x < npx;
    const int64_t y = valid ? labels[p0 + threadIdx.x] : -1;   // (issued before the staging: one memory latency per tile, not two)
    int row = 0;
    if (STAGED) {
      const int len = npx * C;
      const int head = (int)((s0 + mis) & 3);                  // floats between the 16-byte boundary below the span and its start
      __syncthreads();                                         // the previous tile's rows have been read
      for (int i = threadIdx.x * 4; i < head + len; i += TPB * 4) {
        if (i >= head && i + 4 <= head + len) {
          *(float4*)(smem + i) = *(const float4*)(logits + (s0 - head + i));
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (i + j >= head && i + j < head + len) smem[i + j] = logits[s0 - head + i + j];
        }
      }
      __syncthreads();
      row = head + threadIdx.x * C;
    }
    const bool labelled = valid && y >= 0 && y < (int64_t)K;
    const int yi = labelled ? (int)y : -1;
    bool counted = false;
    float nll = 0.f, brier = 0.f;
    if (valid && !labelled) atomicAdd(ints + 2 * B + K, 1ull);
    if (labelled) {
      float z[KK], e[KK];
#pragma unroll
      for (int k = 0; k < KK; ++k) {
        if (STAGED) z[k] = k < K ? smem[row + k] : 0.f;
        else z[k] = k < K ? logits[s0 + (int64_t)threadIdx.x * C + k] : 0.f;
      }
      // u = beta z is rounded on its own (__fmul_rn is never contracted into the subtraction of m below); at beta == 1.0f the
      // product is z itself, bit for bit
#pragma unroll
      for (int k = 0; k < KK; ++k) e[k] = __fmul_rn(beta, z[k]);
      float m = e[0];
#pragma unroll
      for (int k = 1; k < KK; ++k)
        if (k < K) m = fmaxf(m, e[k]);
      float s = 0.f, dy = 0.f;                                 // dy = u_y - m
#pragma unroll
      for (int k = 0; k < KK; ++k)
        if (k < K) {
          const float d = e[k] - m;
          if (k == yi) dy = d;
          e[k] = expf(d);
          s = k ? s + e[k] : e[k];
        }
      float best = 0.f, ez = 0.f, ezz = 0.f;
      int arg = 0;
#pragma unroll
      for (int k = 0; k < KK; ++k)
        if (k < K) {
          const float p = e[k] / s;
          if (k == 0) best = p;
          else if (p > best || (p != p && best == best)) { best = p; arg = k; }   // NaN wins, like torch (k_argmax_channels)
          const float d = p - (k == yi ? 1.f : 0.f);
          brier += d * d;
          ez += p * z[k];
          ezz += p * (z[k] * z[k]);
        }
      const float conf = best;
      if (!(fabsf(conf) <= 3.4028234663852886e38f)) {          // NaN or Inf
        atomicAdd(ints + 2 * B + K + 1, 1ull);
      } else {
        counted = true;
        const unsigned long long ok = arg == yi ? 1ull : 0ull;
        const int bin = min(B - 1, (int)(conf * bf));
        atomicAdd(ints + 2 * bin, 1ull | (ok << 32));
        atomicAdd(ints + 2 * bin + 1, (unsigned long long)(long long)(conf * CONF_SCALE));
        atomicAdd(ints + 2 * B + yi, 1ull | (ok << 32));
        nll = logf(s) - dy;
        float zy = 0.f;
#pragma unroll
        for (int k = 0; k < KK; ++k)
          if (k == yi) zy = z[k];
        ag += (double)(ez - zy);
        ah += (double)fmaxf(ezz - ez * ez, 0.f);
      }
    }
    if (KT) {
#pragma unroll
      for (int k = 0; k < KA; ++k) {
        const bool mine = counted && yi == k;
        an[k] += mine ? (double)nll : 0.0;
        ab[k] += mine ? (double)brier : 0.0;
      }
    } else {
      unsigned long long rem = __ballot(counted);
      while (rem) {                                            // (wave-uniform) one round per true class present in the wave
        const int k = __shfl(yi, __ffsll((long long)rem) - 1, 64);
        const bool mine = counted && yi == k;
        const double a = wave_sum(mine ? (double)nll : 0.0), b = wave_sum(mine ? (double)brier : 0.0);
        if (lane == 0) { wrow[2 * k] += a; wrow[2 * k + 1] += b; }
        rem &= ~__ballot(mine);
      }
    }
  }
  if (KT) {
#pragma unroll
    for (int k = 0; k < KA; ++k) {
      const double a = wave_sum(an[k]), b = wave_sum(ab[k]);
      if (lane == 0) { wrow[2 * k] = a; wrow[2 * k + 1] = b; }
    }
  }
  ag = wave_sum(ag);
  ah = wave_sum(ah);
  if (lane == 0) { wrow[2 * K] = ag; wrow[2 * K + 1] = ah; }
  __syncthreads();
  const int L = calib_len(K, B);
  unsigned long long* mine = part + (size_t)blockIdx.x * L;
  for (int i = threadIdx.x; i < L; i += TPB) {
    unsigned long long v;
    int fslot = -1;                                            // the float sum of this slot, if it is one
    if (i < 3 * B) {
      const int b = i / 3, j = i - 3 * b;
      v = j == 1 ? ints[2 * b + 1] : j == 0 ? (ints[2 * b] & 0xffffffffull) : (ints[2 * b] >> 32);
    } else if (i < 3 * B + 4 * K) {
      const int k = (i - 3 * B) >> 2, j = (i - 3 * B) & 3;
      v = j == 0 ? (ints[2 * B + k] & 0xffffffffull) : (ints[2 * B + k] >> 32);
      if (j >= 2) fslot = 2 * k + j - 2;
    } else {
      const int j = i - 3 * B - 4 * K;
      v = ints[2 * B + K + (j & 1)];
      if (j < 2) fslot = 2 * K + j;
    }
    if (fslot >= 0) {
      double t = wsum[fslot];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) t += wsum[(size_t)w * nflt + fslot];
      v = (unsigned long long)__double_as_longlong(t);
    }
    mine[i] = v;
  }
}

__global__ void __launch_bounds__(FIN_TPB)
k_calibration_finish(const unsigned long long* __restrict__ part, double* __restrict__ out, int G, int K, int B) {
  const int L = calib_len(K, B);
  const int i = blockIdx.x * FIN_TPB + threadIdx.x;
  if (i >= L) return;
  const bool is_float = i >= 3 * B && (i < 3 * B + 4 * K ? ((i - 3 * B) & 3) >= 2 : i - 3 * B - 4 * K < 2);
  double total;
  double tf = 0.0;
  long long ti = 0;
  for (int g0 = 0; g0 < G; g0 += FIN_UNR) {
    unsigned long long v[FIN_UNR];
#pragma unroll
    for (int u = 0; u < FIN_UNR; ++u) v[u] = g0 + u < G ? part[(size_t)(g0 + u) * L + i] : 0ull;
#pragma unroll
    for (int u = 0; u < FIN_UNR; ++u)
      if (g0 + u < G) {                                        // (in workgroup order, whatever the unrolling)
        if (is_float) tf += __longlong_as_double((long long)v[u]);
        else ti += (long long)v[u];
      }
  }
  if (is_float) {
    total = tf;
  } else {
    total = (double)ti;
    if (i < 3 * B && i % 3 == 1) total *= 1.0 / 268435456.0;   // the sum of conf: exact below 2^53
  }
  out[i] += total;
}

bool calib_args_ok(int N, int H, int W, int C, int K, int B) {
  return N >= 0 && N <= SMSUT_CALIB_MAX_SLICES && H >= 1 && W >= 1 && H <= SMSUT_CALIB_MAX_DIM && W <= SMSUT_CALIB_MAX_DIM && K >= 1 &&
         K <= C && K <= MAXK && B >= 1 && B <= MAXB;
}

}  // namespace

extern "C" {

int64_t smsut_calibration_ws(int N, int H, int W, int C, int K, int B) {
  if (!calib_args_ok(N, H, W, C, K, B)) return -1;
  return (int64_t)calib_grid((int64_t)N * H * W) * calib_len(K, B) * (int64_t)sizeof(unsigned long long);
}

int smsut_calibration_stats(const float* logits, const int64_t* labels, double* out, void* workspace, int N, int H, int W, int C, int K,
                            int B, float beta, void* stream) {
  SMSUT_REQUIRE(calib_args_ok(N, H, W, C, K, B));
  SMSUT_REQUIRE(beta > 0.f && beta <= 3.4028234663852886e38f);
  if (N == 0) return SMSUT_OK;
  SMSUT_REQUIRE(logits && labels && out && workspace && ((uintptr_t)logits & 3) == 0);
  const int64_t P = (int64_t)N * H * W;
  const int grid = calib_grid(P);
  const bool staged = C <= STAGE_MAXC;
  const size_t lds = (staged ? (size_t)((TPB * C + 8 + 3) & ~3) * sizeof(float) : 0) + (size_t)(2 * B + K + 2) * sizeof(unsigned long long) +
                     (size_t)WAVES * (2 * K + 2) * sizeof(double);
  unsigned long long* part = (unsigned long long*)workspace;
#define CAL_L(KT, ST) k_calibration<KT, ST><<<grid, TPB, lds, (hipStream_t)stream>>>(logits, labels, part, P, C, K, B, beta)
#define CAL_K(KT) do { if (staged) CAL_L(KT, true); else CAL_L(KT, false); } while (0)
  switch (K) { case 2: CAL_K(2); break; case 3: CAL_K(3); break; case 4: CAL_K(4); break; case 5: CAL_K(5); break;
               default: CAL_K(0); }
#undef CAL_K
#undef CAL_L
  SMSUT_LAUNCH_CHECK();
  k_calibration_finish<<<(calib_len(K, B) + FIN_TPB - 1) / FIN_TPB, FIN_TPB, 0, (hipStream_t)stream>>>(part, out, grid, K, B);
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

}  // extern "C"
