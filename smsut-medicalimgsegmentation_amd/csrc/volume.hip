// Volume preparation on the device (data_pprocess/volume.py): cubic B-spline prefilter, spline / nearest-neighbour resampling into a
// cropped window, exact order statistics and the 8-bit intensity window.  Arrays are dense [D][H][W] = [z][y][x].
//
// Index map (ONE definition, vol_coord below): output index i of an axis reads the source at the continuous index
//   x = ((i + start) * num) / den - offset          fp64: an exact integer product, one division, one subtraction
// and the point is inside iff -0.5 <= x < n - 0.5 on every axis (n = the source's length); outside points are 0.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace {

constexpr int VOL_MAX_DIM = 4096;
constexpr int64_t VOL_MAX_VOXELS = 2147483647LL;
constexpr int VOL_BLOCK = 256;

bool vol_dims_ok(int d, int h, int w) {
  return d >= 1 && h >= 1 && w >= 1 && d <= VOL_MAX_DIM && h <= VOL_MAX_DIM && w <= VOL_MAX_DIM &&
         (int64_t)d * h * w <= VOL_MAX_VOXELS;
}

// whole-sample mirror: -1 -> 1, n -> n - 2, period 2n - 2 (n >= 2)
__host__ __device__ __forceinline__ int vol_mirror(int j, int n) {
  const int p = 2 * n - 2;
  int m = j % p;
  if (m < 0) m += p;
  return m < n ? m : p - m;
}

// ---------------------------------------------------------------------------------------------- B-spline prefilter
// The interpolation coefficients of a line v under mirror boundaries solve A c = v, A = circulant-like (1/6, 4/6, 1/6).  On the
// mirrored (2n-2 periodic) extension that is the convolution with the inverse filter's impulse response
//   h[k] = -6 z / (1 - z^2) * z^|k|,  z = sqrt(3) - 2,
// truncated at |k| <= BSP_K: the dropped tail is 2 h[0] |z|^(K+1) / (1 - |z|) = 3.4e-9 of max |v| at K = 15, below half an fp32
// ulp of the result's scale.  Every output is one fixed-order fp64 sum of 2K+1 products, rounded once to fp32 per axis: fully
// parallel, no recursion along the line, bitwise reproducible.
constexpr int BSP_K = 15;
constexpr int BSP_TAPS = 2 * BSP_K + 1;
struct BspTaps { double h[BSP_K + 1]; };

BspTaps bsp_taps() {
  BspTaps t;
  const double z = std::sqrt(3.0) - 2.0;
  double p = -6.0 * z / (1.0 - z * z);
  for (int k = 0; k <= BSP_K; ++k) { t.h[k] = p; p *= z; }
  return t;
}

// fixed order: the outermost (smallest) pair first, the centre tap last
__device__ __forceinline__ float bsp_dot(const float* s, int stride, const BspTaps& t) {
  double acc = 0.0;
#pragma unroll
  for (int k = BSP_K; k >= 1; --k)
    acc = fma(t.h[k], (double)s[(BSP_K - k) * stride] + (double)s[(BSP_K + k) * stride], acc);
  acc = fma(t.h[0], (double)s[BSP_K * stride], acc);
  return (float)acc;
}

// Lines along x (contiguous): one workgroup item = BSP_TX outputs of one row.  The tile and its mirrored halo go through LDS with
// the lanes along x (coalesced), every thread then reads 2K+1 consecutive words (conflict-free).
constexpr int BSP_TX = VOL_BLOCK;
__global__ __launch_bounds__(VOL_BLOCK) void bsp_filter_x(const float* __restrict__ in, float* __restrict__ out, int64_t rows, int n,
                                                          BspTaps taps) {
  __shared__ float s[BSP_TX + 2 * BSP_K];
  const int tiles = (n + BSP_TX - 1) / BSP_TX;
  const int64_t items = rows * tiles;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {       // (uniform: barriers inside)
    const int64_t row = it / tiles;
    const int x0 = (int)(it - row * tiles) * BSP_TX;
    const float* line = in + row * n;
    for (int k = threadIdx.x; k < BSP_TX + 2 * BSP_K; k += VOL_BLOCK) s[k] = line[vol_mirror(x0 + k - BSP_K, n)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x < n) out[row * n + x] = bsp_dot(s + threadIdx.x, 1, taps);
    __syncthreads();
  }
}

// Lines along y or z: the volume is [outer][n][inner] with inner > 1 contiguous.  One item = BSP_TL outputs along the line for 64
// adjacent inner positions; lanes run along inner for the loads, the stores and the LDS reads (row stride 64 words: no conflict).
constexpr int BSP_TL = 64, BSP_TI = 64;
__global__ __launch_bounds__(VOL_BLOCK) void bsp_filter_s(const float* __restrict__ in, float* __restrict__ out, int outer, int n,
                                                          int64_t inner, BspTaps taps) {
  __shared__ float s[(BSP_TL + 2 * BSP_K) * BSP_TI];
  const int64_t ti = (inner + BSP_TI - 1) / BSP_TI;
  const int tl = (n + BSP_TL - 1) / BSP_TL;
  const int64_t items = (int64_t)outer * tl * ti;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {       // (uniform: barriers inside)
    const int64_t i0 = (it % ti) * BSP_TI;
    const int64_t r = it / ti;
    const int l0 = (int)(r % tl) * BSP_TL;
    const int o = (int)(r / tl);
    const int64_t base = (int64_t)o * n * inner;
    const int64_t i = i0 + lane;
    const int rows_needed = min(BSP_TL, n - l0) + 2 * BSP_K;
    if (i < inner)
      for (int k = wv; k < rows_needed; k += VOL_BLOCK / 64) s[k * BSP_TI + lane] = in[base + (int64_t)vol_mirror(l0 + k - BSP_K, n) * inner + i];
    __syncthreads();
    if (i < inner)
      for (int k = wv; k < BSP_TL; k += VOL_BLOCK / 64) {
        const int l = l0 + k;
        if (l < n) out[base + (int64_t)l * inner + i] = bsp_dot(s + k * BSP_TI + lane, BSP_TI, taps);
      }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- resampling
struct AxisMap { int n_out, n_src, num, den, start, offset; };
struct VolMap { AxisMap a[3]; };      // z, y, x

__device__ __forceinline__ double vol_coord(const AxisMap& m, int i) {
  const double q = __ddiv_rn((double)((int64_t)(i + m.start) * (int64_t)m.num), (double)m.den);
  return __dsub_rn(q, (double)m.offset);
}
__device__ __forceinline__ bool vol_inside(double x, int n) { return x >= -0.5 && x < (double)n - 0.5; }

// Per output index of each axis: the four mirror-folded coefficient indices (idx[0] = -1 outside) and the four cubic B-spline
// weights in fp64 of t = x - floor(x); taps at floor(x) - 1 .. floor(x) + 2.
struct CubicTap { int idx[4]; double w[4]; };

__global__ void cubic_tables(CubicTap* __restrict__ tab, VolMap map) {
  const int total = map.a[0].n_out + map.a[1].n_out + map.a[2].n_out;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < total; k += gridDim.x * blockDim.x) {
    int ax = 0, i = k;
    if (i >= map.a[0].n_out) { i -= map.a[0].n_out; ax = 1; }
    if (ax == 1 && i >= map.a[1].n_out) { i -= map.a[1].n_out; ax = 2; }
    const AxisMap m = map.a[ax];
    const double x = vol_coord(m, i);
    CubicTap c;
    if (!vol_inside(x, m.n_src)) {
      for (int j = 0; j < 4; ++j) { c.idx[j] = -1; c.w[j] = 0.0; }
    } else {
      const double f = floor(x), t = x - f, u = 1.0 - t;
      const int b = (int)f;
      c.w[0] = u * u * u / 6.0;
      c.w[1] = (4.0 - 6.0 * t * t + 3.0 * t * t * t) / 6.0;
      c.w[2] = (4.0 - 6.0 * u * u + 3.0 * u * u * u) / 6.0;
      c.w[3] = t * t * t / 6.0;
      for (int j = 0; j < 4; ++j) c.idx[j] = m.n_src > 1 ? vol_mirror(b - 1 + j, m.n_src) : 0;
    }
    tab[k] = c;
  }
}

// fused 64-tap evaluation, one thread per output voxel of the cropped window, lanes along x; fp64 accumulation in the fixed order
// z (y (x)), rounded once
__global__ __launch_bounds__(VOL_BLOCK) void resample_cubic(const float* __restrict__ coef, float* __restrict__ out,
                                                            const CubicTap* __restrict__ tab, int od, int oh, int ow, int sh, int sw) {
  const int64_t total = (int64_t)od * oh * ow;
  const CubicTap* tz = tab;
  const CubicTap* ty = tab + od;
  const CubicTap* tx = tab + od + oh;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % ow);
    const int64_t r = i / ow;
    const int y = (int)(r % oh), z = (int)(r / oh);
    const CubicTap cz = tz[z], cy = ty[y], cx = tx[x];
    float v = 0.f;
    if (cz.idx[0] >= 0 && cy.idx[0] >= 0 && cx.idx[0] >= 0) {
      double az = 0.0;
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        double ay = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const float* row = coef + ((int64_t)cz.idx[a] * sh + cy.idx[b]) * sw;
          double ax = 0.0;
#pragma unroll
          for (int c = 0; c < 4; ++c) ax = fma(cx.w[c], (double)row[cx.idx[c]], ax);
          ay = fma(cy.w[b], ax, ay);
        }
        az = fma(cz.w[a], ay, az);
      }
      v = (float)az;
    }
    out[i] = v;
  }
}

// nearest neighbour: floor(x + 0.5) per axis (halves round up), -1 outside
__global__ void nearest_tables(int* __restrict__ tab, VolMap map) {
  const int total = map.a[0].n_out + map.a[1].n_out + map.a[2].n_out;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < total; k += gridDim.x * blockDim.x) {
    int ax = 0, i = k;
    if (i >= map.a[0].n_out) { i -= map.a[0].n_out; ax = 1; }
    if (ax == 1 && i >= map.a[1].n_out) { i -= map.a[1].n_out; ax = 2; }
    const AxisMap m = map.a[ax];
    const double x = vol_coord(m, i);
    int j = -1;
    if (vol_inside(x, m.n_src)) j = min(max((int)floor(x + 0.5), 0), m.n_src - 1);
    tab[k] = j;
  }
}

__global__ __launch_bounds__(VOL_BLOCK) void resample_nearest(const uint8_t* __restrict__ lab, uint8_t* __restrict__ out,
                                                              const int* __restrict__ tab, const uint8_t* __restrict__ lut, int od,
                                                              int oh, int ow, int sh, int sw) {
  const int64_t total = (int64_t)od * oh * ow;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % ow);
    const int64_t r = i / ow;
    const int y = (int)(r % oh), z = (int)(r / oh);
    const int jz = tab[z], jy = tab[od + y], jx = tab[od + oh + x];
    uint8_t v = 0;
    if (jz >= 0 && jy >= 0 && jx >= 0) {
      v = lab[((int64_t)jz * sh + jy) * sw + jx];
      if (lut) v = lut[v];
    }
    out[i] = v;
  }
}

bool axis_ok(const AxisMap& m) {
  return m.n_out >= 1 && m.n_out <= VOL_MAX_DIM && m.n_src >= 1 && m.n_src <= VOL_MAX_DIM && m.num >= 1 && m.num <= VOL_MAX_DIM &&
         m.den >= 1 && m.den <= VOL_MAX_DIM && m.start >= 0 && m.start <= VOL_MAX_DIM && m.offset >= 0 && m.offset <= VOL_MAX_DIM;
}

// the entry points' per-axis scalars as one map; false for anything outside the limits
bool resample_args(VolMap& m, int sd, int sh, int sw, int od, int oh, int ow, int num_z, int num_y, int num_x, int den_z, int den_y,
                   int den_x, int start_z, int start_y, int start_x, int off_z, int off_y, int off_x) {
  m.a[0] = AxisMap{od, sd, num_z, den_z, start_z, off_z};
  m.a[1] = AxisMap{oh, sh, num_y, den_y, start_y, off_y};
  m.a[2] = AxisMap{ow, sw, num_x, den_x, start_x, off_x};
  return vol_dims_ok(sd, sh, sw) && vol_dims_ok(od, oh, ow) && axis_ok(m.a[0]) && axis_ok(m.a[1]) && axis_ok(m.a[2]);
}

// ---------------------------------------------------------------------------------------------- order statistics
// Exact selection of up to OS_MAX_RANKS sorted ranks among n finite floats: an MSD radix select over order-preserving 32-bit keys,
// four levels of 8 bits.  Level L histograms the byte below the prefix chosen so far, per rank, over the values whose higher bits
// equal that rank's prefix (level 0: one histogram for all ranks); a one-block step extends every prefix and reduces every rank to
// its rank inside the chosen bin.  After level 3 the prefix IS the key.  Integer counts and integer atomics only: the result does
// not depend on the order of arrival; every loop's trip count is fixed by n.
constexpr int OS_MAX_RANKS = 8;
constexpr int OS_BINS = 256;
constexpr int OS_LEVELS = 4;
constexpr int OS_CTRL = 2 * OS_MAX_RANKS;                         // prefix[8], rank-in-bin[8]
constexpr int OS_WORDS = OS_CTRL + OS_LEVELS * OS_MAX_RANKS * OS_BINS;
constexpr int OS_GRID_CAP = 1024;
struct OsRanks { unsigned r[OS_MAX_RANKS]; };

__device__ __forceinline__ unsigned os_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float os_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// one value into an LDS histogram: the lanes that hold the first pending lane's bin add their count once (real volumes are
// dominated by a few values -- air, zero padding -- whose 64 atomics would serialise on one word), the rest go one by one
__device__ __forceinline__ void os_hist_add(unsigned* h, int bin, bool valid) {
  const int lane = threadIdx.x & 63;
  bool rem = valid;
  if (rem) {
    const int k = __builtin_amdgcn_readfirstlane(bin);
    if (bin == k) {
      const unsigned long long same = __ballot(1);
      if (lane == __ffsll((long long)same) - 1) atomicAdd(&h[k], (unsigned)__popcll(same));
      rem = false;
    }
  }
  if (rem) atomicAdd(&h[bin], 1u);
}

template <int LEVEL>
__global__ __launch_bounds__(VOL_BLOCK) void os_hist(const float* __restrict__ v, int64_t n, int nr, unsigned* ws) {
  constexpr int NH = LEVEL ? OS_MAX_RANKS : 1;
  constexpr int SHIFT = 24 - 8 * LEVEL;
  __shared__ unsigned h[NH * OS_BINS];
  __shared__ unsigned prefix[OS_MAX_RANKS];
  for (int k = threadIdx.x; k < NH * OS_BINS; k += VOL_BLOCK) h[k] = 0;
  if (threadIdx.x < OS_MAX_RANKS) prefix[threadIdx.x] = ws[threadIdx.x];
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned key = os_key(v[i]);
    const int bin = (int)((key >> SHIFT) & 255u);
    if (LEVEL == 0) {
      os_hist_add(h, bin, true);
    } else {
      const unsigned hi = key >> (SHIFT + 8);
      for (int r = 0; r < nr; ++r)                                  // (uniform)
        os_hist_add(h + r * OS_BINS, bin, hi == prefix[r]);
    }
  }
  __syncthreads();
  unsigned* g = ws + OS_CTRL + LEVEL * OS_MAX_RANKS * OS_BINS;
  for (int k = threadIdx.x; k < (LEVEL ? nr : 1) * OS_BINS; k += VOL_BLOCK)
    if (h[k]) atomicAdd(g + k, h[k]);
}

// thread r walks rank r's 256 bins: the bin that holds the rank, and the rank inside it
template <int LEVEL>
__global__ void os_step(unsigned* ws, OsRanks ranks, int nr, float* __restrict__ out) {
  const int r = threadIdx.x;
  if (r >= nr) return;
  const unsigned* hist = ws + OS_CTRL + LEVEL * OS_MAX_RANKS * OS_BINS + (LEVEL ? r * OS_BINS : 0);
  const unsigned want = LEVEL ? ws[OS_MAX_RANKS + r] : ranks.r[r];
  unsigned acc = 0, bin = OS_BINS - 1, inside = 0;
  bool found = false;
  for (int b = 0; b < OS_BINS; ++b) {
    const unsigned c = hist[b];
    if (!found && want - acc < c) { bin = (unsigned)b; inside = want - acc; found = true; }
    if (!found) acc += c;
  }
  const unsigned p = ((LEVEL ? ws[r] : 0u) << 8) | bin;
  if (LEVEL == OS_LEVELS - 1) {
    out[r] = os_unkey(p);
  } else {
    ws[r] = p;
    ws[OS_MAX_RANKS + r] = inside;
  }
}

// ---------------------------------------------------------------------------------------------- 8-bit window
// (uint8)((min(max(x, lo), hi) - lo) / (hi - lo) * 255.0f): fp32, this order, IEEE division, truncation; all zeros when hi == lo
__device__ __forceinline__ unsigned window_one(float x, float lo, float hi, float span) {
  const float c = fminf(fmaxf(x, lo), hi);
  const float q = __fmul_rn(__fdiv_rn(__fsub_rn(c, lo), span), 255.0f);
  return span == 0.f ? 0u : ((unsigned)(int)q & 255u);
}

__global__ __launch_bounds__(VOL_BLOCK) void window_u8(const float* __restrict__ v, const float* __restrict__ bounds,
                                                       uint8_t* __restrict__ out, int64_t n) {
  const float lo = bounds[0], hi = bounds[1];
  const float span = __fsub_rn(hi, lo);
  const bool aligned = ((uintptr_t)v % 16 == 0) && ((uintptr_t)out % 4 == 0);       // (a view into a larger tensor may not be)
  const int64_t n4 = aligned ? n / 4 : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < n4; i += stride) {
    const float4 x = reinterpret_cast<const float4*>(v)[i];
    const unsigned p = window_one(x.x, lo, hi, span) | (window_one(x.y, lo, hi, span) << 8) | (window_one(x.z, lo, hi, span) << 16) |
                       (window_one(x.w, lo, hi, span) << 24);
    reinterpret_cast<unsigned*>(out)[i] = p;
  }
  for (int64_t i = 4 * n4 + t0; i < n; i += stride) out[i] = (uint8_t)window_one(v[i], lo, hi, span);
}

}  // namespace

extern "C" {

int64_t smsut_bspline_ws(int d, int h, int w) {
  if (!vol_dims_ok(d, h, w)) return -1;
  return (int64_t)d * h * w * 4;
}

int smsut_bspline_coefficients(const float* vol, float* out, void* workspace, int d, int h, int w, void* stream) {
  SMSUT_REQUIRE(vol_dims_ok(d, h, w) && vol && out && workspace);
  hipStream_t st = (hipStream_t)stream;
  const int64_t N = (int64_t)d * h * w;
  const BspTaps taps = bsp_taps();
  const int passes = (w > 1) + (h > 1) + (d > 1);
  if (passes == 0) {
    hipError_t e = hipMemcpyAsync(out, vol, N * 4, hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? SMSUT_OK : (int)e;
  }
  const float* src = vol;
  int p = 0;
  auto dst_of = [&](int pass) { return ((passes - 1 - pass) & 1) ? (float*)workspace : out; };     // the last pass lands in out
  if (w > 1) {
    float* dst = dst_of(p++);
    const int64_t rows = (int64_t)d * h, items = rows * cdiv64(w, BSP_TX);
    bsp_filter_x<<<(int)std::min<int64_t>(items, 4096), VOL_BLOCK, 0, st>>>(src, dst, rows, w, taps);
    SMSUT_LAUNCH_CHECK();
    src = dst;
  }
  if (h > 1) {
    float* dst = dst_of(p++);
    const int64_t items = (int64_t)d * cdiv64(h, BSP_TL) * cdiv64(w, BSP_TI);
    bsp_filter_s<<<(int)std::min<int64_t>(items, 4096), VOL_BLOCK, 0, st>>>(src, dst, d, h, (int64_t)w, taps);
    SMSUT_LAUNCH_CHECK();
    src = dst;
  }
  if (d > 1) {
    float* dst = dst_of(p++);
    const int64_t items = cdiv64(d, BSP_TL) * cdiv64((int64_t)h * w, BSP_TI);
    bsp_filter_s<<<(int)std::min<int64_t>(items, 4096), VOL_BLOCK, 0, st>>>(src, dst, 1, d, (int64_t)h * w, taps);
    SMSUT_LAUNCH_CHECK();
  }
  return SMSUT_OK;
}

int64_t smsut_resample_ws(int od, int oh, int ow) {
  if (!vol_dims_ok(od, oh, ow)) return -1;
  return (int64_t)(od + oh + ow) * (int64_t)sizeof(CubicTap);
}

int smsut_resample_volume(const float* coef, float* out, void* workspace, int sd, int sh, int sw, int od, int oh, int ow, int num_z,
                          int num_y, int num_x, int den_z, int den_y, int den_x, int start_z, int start_y, int start_x, int off_z,
                          int off_y, int off_x, void* stream) {
  VolMap m;
  SMSUT_REQUIRE(resample_args(m, sd, sh, sw, od, oh, ow, num_z, num_y, num_x, den_z, den_y, den_x, start_z, start_y, start_x, off_z,
                              off_y, off_x) && coef && out && workspace);
  hipStream_t st = (hipStream_t)stream;
  CubicTap* tab = (CubicTap*)workspace;
  cubic_tables<<<ew_grid(od + oh + ow), VOL_BLOCK, 0, st>>>(tab, m);
  SMSUT_LAUNCH_CHECK();
  resample_cubic<<<ew_grid((int64_t)od * oh * ow), VOL_BLOCK, 0, st>>>(coef, out, tab, od, oh, ow, sh, sw);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

int smsut_resample_labels(const uint8_t* lab, uint8_t* out, void* workspace, const uint8_t* lut /*nullable*/, int sd, int sh, int sw,
                          int od, int oh, int ow, int num_z, int num_y, int num_x, int den_z, int den_y, int den_x, int start_z,
                          int start_y, int start_x, int off_z, int off_y, int off_x, void* stream) {
  VolMap m;
  SMSUT_REQUIRE(resample_args(m, sd, sh, sw, od, oh, ow, num_z, num_y, num_x, den_z, den_y, den_x, start_z, start_y, start_x, off_z,
                              off_y, off_x) && lab && out && workspace);
  hipStream_t st = (hipStream_t)stream;
  int* tab = (int*)workspace;
  nearest_tables<<<ew_grid(od + oh + ow), VOL_BLOCK, 0, st>>>(tab, m);
  SMSUT_LAUNCH_CHECK();
  resample_nearest<<<ew_grid((int64_t)od * oh * ow), VOL_BLOCK, 0, st>>>(lab, out, tab, lut, od, oh, ow, sh, sw);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

int64_t smsut_order_statistics_ws(int64_t n, int nr) {
  if (n < 1 || n > VOL_MAX_VOXELS || nr < 1 || nr > OS_MAX_RANKS) return -1;
  return (int64_t)OS_WORDS * 4;
}

int smsut_order_statistics(const float* v, float* out, void* workspace, int64_t n, int nr, int64_t r0, int64_t r1, int64_t r2,
                           int64_t r3, int64_t r4, int64_t r5, int64_t r6, int64_t r7, void* stream) {
  SMSUT_REQUIRE(smsut_order_statistics_ws(n, nr) > 0 && v && out && workspace);
  const int64_t rk[OS_MAX_RANKS] = {r0, r1, r2, r3, r4, r5, r6, r7};
  OsRanks ranks;
  for (int k = 0; k < OS_MAX_RANKS; ++k) {
    SMSUT_REQUIRE(k >= nr || (rk[k] >= 0 && rk[k] < n));
    ranks.r[k] = k < nr ? (unsigned)rk[k] : 0u;
  }
  hipStream_t st = (hipStream_t)stream;
  unsigned* ws = (unsigned*)workspace;
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)OS_WORDS * 4, st);
  if (e != hipSuccess) return (int)e;
  const int grid = (int)std::min<int64_t>(cdiv64(n, VOL_BLOCK), OS_GRID_CAP);
  os_hist<0><<<grid, VOL_BLOCK, 0, st>>>(v, n, nr, ws);
  os_step<0><<<1, 64, 0, st>>>(ws, ranks, nr, out);
  os_hist<1><<<grid, VOL_BLOCK, 0, st>>>(v, n, nr, ws);
  os_step<1><<<1, 64, 0, st>>>(ws, ranks, nr, out);
  os_hist<2><<<grid, VOL_BLOCK, 0, st>>>(v, n, nr, ws);
  os_step<2><<<1, 64, 0, st>>>(ws, ranks, nr, out);
  os_hist<3><<<grid, VOL_BLOCK, 0, st>>>(v, n, nr, ws);
  os_step<3><<<1, 64, 0, st>>>(ws, ranks, nr, out);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

int smsut_window_u8(const float* v, const float* bounds, uint8_t* out, int64_t n, void* stream) {
  SMSUT_REQUIRE(n >= 1 && n <= VOL_MAX_VOXELS && v && bounds && out);
  window_u8<<<ew_grid(cdiv64(n, 4)), VOL_BLOCK, 0, (hipStream_t)stream>>>(v, bounds, out, n);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

}  // extern "C"
