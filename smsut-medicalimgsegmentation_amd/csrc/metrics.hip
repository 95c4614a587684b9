// Test-phase metrics (reference misc/utils.py:18-36 connected_components, :206-283 get_all_matrix with medpy's dc / assd):
//   smsut_cc_filter      connected-component cleanup of every class 1..n_cls in one labelling pass (3-D 18-neighbour or
//                        per-slice 8-neighbour union-find, Playne & Hawick 2018), components of <= 10 % of their class dropped;
//   smsut_surface_stats  per label: Dice counts and, both ways, the border-voxel count and the fp64 sum of the exact Euclidean
//                        distances from one mask's border to the other's (separable squared EDT: brute-force minimum over each
//                        line's finite entries staged in LDS for x and y, the z pass fused with the gather);
//   smsut_surface_hd     per label: the border-voxel counts, the largest squared distance each way and two order statistics
//                        of the pooled squared distances (Hausdorff and its percentile, medpy's hd / hd95), by an exact
//                        two-level radix select over LDS histograms;
//   smsut_surface_stats_sp / smsut_surface_hd_sp  the same two with an anisotropic voxel spacing: fp64 weighted squared
//                        distances through the same passes, and a five-level radix select over the doubles' bit patterns.
// No float atomics: fp64 partials per block, reduced in a fixed order; the histograms take integer atomics only (bitwise
// reproducible).
#include <algorithm>

#include "common.h"

namespace {

constexpr int CC_BLOCK = 256;
constexpr int SURF_MAX_DIM = 4096;      // LDS line length; also keeps every finite squared distance below 3 * 4095^2 < 2^26
constexpr int SURF_INF = 1 << 30;       // "no feature on this line"; INF + 4095^2 still fits an int
constexpr int SURF_BLOCK = 256;
constexpr int SURF_GRID_CAP = 2048;     // gather blocks (a fixed function of N: the reduction order does not depend on the device)

// ---------------------------------------------------------------------------------------------- cleanup: union-find
// Parent indices only decrease (par[i] <= i, written by atomicMin alone), so every find walk is strictly decreasing and ends
// after at most i + 1 steps; a union retries only when its larger root stopped being a root, and then the larger of the two
// candidates strictly decreases.  Both loops are still capped at N iterations: hitting the cap sets the error word.
// Parents are read with relaxed agent-scope loads (the XCDs' L2s are not coherent with each other); the trees are consumed
// by other workgroups only after a kernel boundary.
__device__ __forceinline__ int par_load(const int* par, int i) {
  return __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x with path halving (x hops over its parent); false when the iteration cap was hit
__device__ bool cc_find(int* par, int x, int64_t cap, int& root) {
  int p = par_load(par, x);
  for (int64_t it = 0; it < cap; ++it) {
    if (p == x) {
      root = x;
      return true;
    }
    const int gp = par_load(par, p);
    if (gp != p) atomicMin(par + x, gp);
    x = p;
    p = gp;
  }
  return false;
}

__device__ bool cc_union(int* par, int a, int b, int64_t cap) {
  for (int64_t it = 0; it < cap; ++it) {
    if (!cc_find(par, a, cap, a) || !cc_find(par, b, cap, b)) return false;
    if (a == b) return true;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(par + a, b);     // hang the larger root under the smaller one
    if (old == a) return true;
    a = old;                                   // a had been hung elsewhere meanwhile: join that tree to b as well
  }
  return false;
}

__device__ __forceinline__ void flag_error(int* err) { atomicOr(err, 1); }

__global__ void cc_init(const uint8_t* __restrict__ in, int* __restrict__ par, int* __restrict__ cnt, int* __restrict__ tot,
                        int* __restrict__ err, int64_t N, int64_t ntot, int n_cls) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t0 == 0) *err = 0;
  for (int64_t i = t0; i < ntot; i += stride) tot[i] = 0;
  for (int64_t i = t0; i < N; i += stride) {
    const int v = in[i];
    par[i] = (v >= 1 && v <= n_cls) ? (int)i : -1;
    cnt[i] = 0;
  }
}

// backward half of the neighbourhood, (dz, dy, dx): rows 0..8 = 18-neighbour 3-D, rows 5..8 = 8-neighbour in-plane
__constant__ int8_t kHalf[9][3] = {{-1, -1, 0}, {-1, 0, -1}, {-1, 0, 0}, {-1, 0, 1}, {-1, 1, 0},
                                   {0, -1, -1}, {0, -1, 0},  {0, -1, 1}, {0, 0, -1}};

__global__ __launch_bounds__(CC_BLOCK) void cc_merge(const uint8_t* __restrict__ in, int* par, int* err, int D, int H, int W,
                                                     int n_cls, int per_slice) {
  const int64_t N = (int64_t)D * H * W;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int v = in[i];
  if (v < 1 || v > n_cls) return;
  const int x = (int)(i % W);
  const int64_t r = i / W;
  const int y = (int)(r % H);
  const int z = (int)(r / H);
  for (int k = per_slice ? 5 : 0; k < 9; ++k) {
    const int zz = z + kHalf[k][0], yy = y + kHalf[k][1], xx = x + kHalf[k][2];
    if (zz < 0 || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
    const int64_t j = ((int64_t)zz * H + yy) * W + xx;
    if (in[j] != v) continue;
    if (!cc_union(par, (int)i, (int)j, N)) {
      flag_error(err);
      return;
    }
  }
}

// arr[key] += 1 for every lane with key >= 0, one atomic per distinct key of the wave (components are mostly wave-uniform)
__device__ __forceinline__ void wave_count(int* arr, int key) {
  uint64_t pending = __ballot(key >= 0);
  while (pending) {
    const int leader = __ffsll((unsigned long long)pending) - 1;
    const int k = __shfl(key, leader);
    const uint64_t same = __ballot(key == k);
    if ((int)__lane_id() == leader) atomicAdd(arr + k, (int)__popcll(same));
    pending &= ~same;
  }
}

// compress every parent to its root (the trees are final after cc_merge) and count component sizes and class totals
__global__ __launch_bounds__(CC_BLOCK) void cc_count(const uint8_t* __restrict__ in, int* par, int* __restrict__ cnt,
                                                     int* __restrict__ tot, int* err, int64_t N, int64_t HW, int n_cls,
                                                     int per_slice) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int root_key = -1, tot_key = -1;
  if (i < N) {
    const int v = in[i];
    if (v >= 1 && v <= n_cls) {
      int root;
      if (cc_find(par, (int)i, N, root)) {
        atomicMin(par + i, root);
        root_key = root;
        tot_key = (int)((per_slice ? (i / HW) * n_cls : 0) + (v - 1));
      } else {
        flag_error(err);
      }
    }
  }
  wave_count(cnt, root_key);
  wave_count(tot, tot_key);
}

__global__ __launch_bounds__(CC_BLOCK) void cc_keep(const uint8_t* in, uint8_t* out, const int* __restrict__ par,
                                                    const int* __restrict__ cnt, const int* __restrict__ tot, int64_t N,
                                                    int64_t HW, int n_cls, int per_slice) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int v = in[i];
  uint8_t o = 0;
  if (v >= 1 && v <= n_cls) {
    const int F = tot[(per_slice ? (i / HW) * n_cls : 0) + (v - 1)];
    if ((double)cnt[par[i]] > 0.1 * (double)F) o = (uint8_t)v;     // the reference's fp64 predicate: size > 0.1 * F
  }
  out[i] = o;
}

struct CcLayout {
  int64_t tot, cnt, par, bytes;     // byte offsets; the error word is the first int
};

CcLayout cc_layout(int D, int H, int W, int n_cls, int per_slice) {
  const int64_t N = (int64_t)D * H * W;
  const int64_t ntot = (int64_t)(per_slice ? D : 1) * n_cls;
  CcLayout l;
  l.tot = 256;
  l.cnt = l.tot + cdiv64(ntot * 4, 256) * 256;
  l.par = l.cnt + cdiv64(N * 4, 256) * 256;
  l.bytes = l.par + N * 4;
  return l;
}

bool dims_ok(int D, int H, int W) {
  return D > 0 && H > 0 && W > 0 && (int64_t)D * H * W < ((int64_t)1 << 31);
}

bool cc_args_ok(int D, int H, int W, int n_cls, int per_slice) {
  return dims_ok(D, H, W) && n_cls >= 1 && n_cls <= 255 && (per_slice == 0 || per_slice == 1) &&
         (int64_t)(per_slice ? D : 1) * n_cls < ((int64_t)1 << 31);
}

// ---------------------------------------------------------------------------------------------- surface distances
// border voxel of label `lab` in m: in the mask with a 6-neighbour outside it (outside the array counts as outside the mask:
// binary_erosion with the cross structure and border value 0); planar = 1 for a 2-D image (no z neighbours at all)
__device__ __forceinline__ bool is_border(const uint8_t* __restrict__ m, int lab, int z, int y, int x, int D, int H, int W,
                                          int planar) {
  const int64_t HW = (int64_t)H * W;
  const int64_t i = (int64_t)z * HW + (int64_t)y * W + x;
  if (m[i] != lab) return false;
  if (y == 0 || y == H - 1 || x == 0 || x == W - 1) return true;
  if (m[i - 1] != lab || m[i + 1] != lab || m[i - W] != lab || m[i + W] != lab) return true;
  if (planar) return false;
  return z == 0 || z == D - 1 || m[i - HW] != lab || m[i + HW] != lab;
}

// pass 1, one block per (z, y) row: squared distance along x to the nearest border voxel of `lab` in fb (SURF_INF: none)
__global__ __launch_bounds__(SURF_BLOCK) void edt_rows(const uint8_t* __restrict__ fb, int lab, int* __restrict__ g, int D,
                                                       int H, int W, int planar) {
  __shared__ int pos[SURF_MAX_DIM];
  __shared__ int npos;
  const int row = blockIdx.x;
  const int z = row / H, y = row % H;
  if (threadIdx.x == 0) npos = 0;
  __syncthreads();
  for (int x = threadIdx.x; x < W; x += blockDim.x)
    if (is_border(fb, lab, z, y, x, D, H, W, planar)) pos[atomicAdd(&npos, 1)] = x;
  __syncthreads();
  const int n = npos;
  int* out = g + (int64_t)row * W;
  for (int x = threadIdx.x; x < W; x += blockDim.x) {
    int best = SURF_INF;
    for (int k = 0; k < n; ++k) {
      const int d = x - pos[k];
      best = min(best, d * d);
    }
    out[x] = best;
  }
}

// pass 2, one block per (z, x) column, in place: g(y) <- min over finite g(y') of g(y') + (y - y')^2
__global__ __launch_bounds__(SURF_BLOCK) void edt_cols(int* g, int H, int W) {
  __shared__ int val[SURF_MAX_DIM];
  __shared__ int pos[SURF_MAX_DIM];
  __shared__ int npos;
  const int z = blockIdx.x / W, x = blockIdx.x % W;
  int* col = g + (int64_t)z * H * W + x;
  if (threadIdx.x == 0) npos = 0;
  __syncthreads();
  for (int y = threadIdx.x; y < H; y += blockDim.x) {
    const int v = col[(int64_t)y * W];
    if (v < SURF_INF) {
      const int k = atomicAdd(&npos, 1);
      val[k] = v;
      pos[k] = y;
    }
  }
  __syncthreads();
  const int n = npos;
  for (int y = threadIdx.x; y < H; y += blockDim.x) {
    int best = SURF_INF;
    for (int k = 0; k < n; ++k) {
      const int d = y - pos[k];
      best = min(best, val[k] + d * d);
    }
    col[(int64_t)y * W] = best;
  }
}

// block sum in a fixed order: butterfly inside each wave, then the waves' totals in wave order
__device__ double block_sum_d(double v, double* red) {
  v = wave_sum_d(v);
  const int wid = threadIdx.x / 64, nw = blockDim.x / 64;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wid] = v;
  __syncthreads();
  double s = 0.0;
  for (int k = 0; k < nw; ++k) s += red[k];
  return s;
}

// pass 3 along z fused with the gather at the border voxels of `lab` in fa and the per-block reduction:
// part[block] = {border voxels, sum of sqrt(d^2)}
__global__ __launch_bounds__(SURF_BLOCK) void edt_gather(const uint8_t* __restrict__ fa, int lab, const int* __restrict__ g,
                                                         double* __restrict__ part, int D, int H, int W, int planar) {
  __shared__ double red[SURF_BLOCK / 64];
  const int64_t HW = (int64_t)H * W, N = HW * D;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double nb = 0.0, sum = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
    const int z = (int)(i / HW);
    const int64_t p = i - z * HW;
    const int y = (int)(p / W), x = (int)(p % W);
    if (!is_border(fa, lab, z, y, x, D, H, W, planar)) continue;
    int best = SURF_INF;
    for (int zz = 0; zz < D; ++zz) {
      const int d = z - zz;
      best = min(best, g[zz * HW + p] + d * d);
    }
    nb += 1.0;
    sum += sqrt((double)best);
  }
  nb = block_sum_d(nb, red);
  sum = block_sum_d(sum, red);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = nb;
    part[2 * blockIdx.x + 1] = sum;
  }
}

__global__ void surf_zero(unsigned long long* cnt, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) cnt[i] = 0;
}

// Dice counts per label: {|P & G|, |P|, |G|} through an LDS histogram per block (integer atomics: order-free)
__global__ __launch_bounds__(SURF_BLOCK) void surf_counts(const uint8_t* __restrict__ pr, const uint8_t* __restrict__ gt,
                                                          unsigned long long* cnt, int64_t N, int n_cls) {
  __shared__ int hist[3 * 255];
  for (int k = threadIdx.x; k < 3 * n_cls; k += blockDim.x) hist[k] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const int a = pr[i], b = gt[i];
    if (a >= 1 && a <= n_cls) {
      atomicAdd(&hist[3 * (a - 1) + 1], 1);
      if (a == b) atomicAdd(&hist[3 * (a - 1)], 1);
    }
    if (b >= 1 && b <= n_cls) atomicAdd(&hist[3 * (b - 1) + 2], 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < 3 * n_cls; k += blockDim.x)
    if (hist[k]) atomicAdd(cnt + k, (unsigned long long)hist[k]);
}

// out[l][7] = {|P&G|, |P|, |G|, border(P), sum d(border P -> border G), border(G), sum d(border G -> border P)};
// block s = 2 * l + dir reduces the partials of set s in a fixed order
__global__ __launch_bounds__(SURF_BLOCK) void surf_final(const unsigned long long* __restrict__ cnt,
                                                         const double* __restrict__ part, double* __restrict__ out, int G) {
  __shared__ double red[SURF_BLOCK / 64];
  const int s = blockIdx.x, l = s / 2, dir = s % 2;
  const double* p = part + (int64_t)s * G * 2;
  double nb = 0.0, sum = 0.0;
  for (int k = threadIdx.x; k < G; k += blockDim.x) {
    nb += p[2 * k];
    sum += p[2 * k + 1];
  }
  nb = block_sum_d(nb, red);
  sum = block_sum_d(sum, red);
  if (threadIdx.x == 0) {
    out[7 * l + 3 + 2 * dir] = nb;
    out[7 * l + 4 + 2 * dir] = sum;
    if (dir == 0)
      for (int k = 0; k < 3; ++k) out[7 * l + k] = (double)cnt[3 * l + k];
  }
}

struct SurfLayout {
  int64_t part, g, bytes;     // byte offsets; the Dice counts come first
  int G;
};

SurfLayout surf_layout(int D, int H, int W, int n_cls) {
  const int64_t N = (int64_t)D * H * W;
  SurfLayout l;
  l.G = (int)std::min<int64_t>(cdiv64(N, SURF_BLOCK), SURF_GRID_CAP);
  l.part = cdiv64((int64_t)3 * n_cls * 8, 256) * 256;
  l.g = l.part + cdiv64((int64_t)2 * n_cls * l.G * 2 * 8, 256) * 256;
  l.bytes = l.g + N * 4;
  return l;
}

bool surf_args_ok(int D, int H, int W, int n_cls, int planar) {
  return dims_ok(D, H, W) && D <= SURF_MAX_DIM && H <= SURF_MAX_DIM && W <= SURF_MAX_DIM && n_cls >= 1 && n_cls <= 255 &&
         (planar == 0 || (planar == 1 && D == 1));
}

int line_block(int len) { return (int)std::min<int64_t>(SURF_BLOCK, cdiv64(len, 64) * 64); }

// ---------------------------------------------------------------------------------------------- Hausdorff / percentile
// Every squared distance is an integer below 2^26, so the maximum and any order statistic of a label's pooled distances are
// exact: a two-level radix select, 13 bits a level, over the dense d^2 buffers the gather leaves (-1 off the border).  Counts
// are unsigned (a pool holds at most 2 * D*H*W < 2^32 entries) and only integer atomics touch them: the result does not
// depend on the order of arrival.
constexpr int HD_SHIFT = 13;
constexpr int HD_BINS = 1 << HD_SHIFT;
constexpr int HD_LIMIT = 1 << (2 * HD_SHIFT);            // finite squared distances lie below it (3 * 4095^2 < 2^26)
constexpr int HD_CTRL = 16;                              // control words of one label, ahead of its three histograms
constexpr int HD_LABEL_WORDS = HD_CTRL + 3 * HD_BINS;    // hist 0: d^2 >> 13; hist 1, 2: d^2 & 8191 inside the bucket of rank lo, hi
constexpr int HD_HIST_ITEMS = 16;                        // buffer entries per thread of a histogram block
constexpr int HD_HIST_GRID_CAP = 1024;
// control words: border voxels per direction, largest d^2 per direction, then (bucket, rank inside it) of the two ranks
enum { HD_N = 0, HD_MAX = 2, HD_SEL = 4 };

static_assert(HD_BINS == 32 * SURF_BLOCK, "hd_select gives every thread of one block 32 bins");
static_assert(3LL * (SURF_MAX_DIM - 1) * (SURF_MAX_DIM - 1) < HD_LIMIT, "two levels must cover every finite squared distance");

__global__ void hd_zero(unsigned* w, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) w[i] = 0;
}

// edt_gather's z pass, keeping every value: d2[i] = squared distance at the border voxels of `lab` in fa, -1 elsewhere;
// part[block] = {border voxels, max d^2} (no global atomics here: thousands of waves on one address serialise in L2)
__global__ __launch_bounds__(SURF_BLOCK) void edt_gather_d2(const uint8_t* __restrict__ fa, int lab, const int* __restrict__ g,
                                                            int* __restrict__ d2, unsigned* __restrict__ part, int D, int H,
                                                            int W, int planar) {
  __shared__ unsigned red[2 * (SURF_BLOCK / 64)];
  const int64_t HW = (int64_t)H * W, N = HW * D;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned nb = 0, mx = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
    const int z = (int)(i / HW);
    const int64_t p = i - z * HW;
    const int y = (int)(p / W), x = (int)(p % W);
    int v = -1;
    if (is_border(fa, lab, z, y, x, D, H, W, planar)) {
      int best = SURF_INF;
      for (int zz = 0; zz < D; ++zz) {
        const int d = z - zz;
        best = min(best, g[zz * HW + p] + d * d);
      }
      v = best;
      nb += 1;
      mx = max(mx, (unsigned)best);     // (>= SURF_INF when the other mask is empty: meaningless then, hd_final writes -1)
    }
    d2[i] = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nb += __shfl_xor(nb, o, 64);
    mx = max(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[2 * (threadIdx.x / 64)] = nb;
    red[2 * (threadIdx.x / 64) + 1] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < SURF_BLOCK / 64; ++k) {
      nb += red[2 * k];
      mx = max(mx, red[2 * k + 1]);
    }
    part[2 * blockIdx.x] = nb;
    part[2 * blockIdx.x + 1] = mx;
  }
}

// One key into the block's LDS histogram.  Segmentations give small distances: nearly every entry of the first level has key 0
// and a handful of keys take the second, so the 64 atomics of a wave would serialise on one address.  As in photo_hist_add
// (photometric.hip), HD_VOTE_ROUNDS values are taken out by vote first: the lanes that hold the first pending lane's key add
// their popcount once; only what is left goes through per-lane atomics.
#ifndef HD_VOTE_ROUNDS
#define HD_VOTE_ROUNDS 1
#endif
__device__ __forceinline__ void hd_hist_add(unsigned* h, int key, bool valid) {
  const int lane = threadIdx.x & 63;
  bool rem = valid;
#pragma unroll
  for (int r = 0; r < HD_VOTE_ROUNDS; ++r) {
    if (rem) {
      const int k = __builtin_amdgcn_readfirstlane(key);
      if (key == k) {
        const unsigned long long same = __ballot(1);          // the active lanes: exactly those that hold k
        if (lane == __ffsll((long long)same) - 1) atomicAdd(&h[k], (unsigned)__popcll(same));
        rem = false;
      }
    }
  }
  if (rem) atomicAdd(&h[key], 1u);
}

// LEVEL 0: histogram of d^2 >> 13 over both directions' buffers; LEVEL 1 / 2: of d^2 & 8191 over the entries of the bucket that
// holds rank lo / hi (level 2 only when the two buckets differ).  A label with an empty mask has no finite d^2 (SURF_INF lies
// beyond the bins and is passed over): its first level stays empty, hd_pick records the zero count and the other levels return.
template <int LEVEL>
__global__ __launch_bounds__(SURF_BLOCK) void hd_hist(const int* __restrict__ d2, int64_t n2, unsigned* ctrl) {
  __shared__ unsigned h[HD_BINS];
  if (LEVEL && (ctrl[HD_N] == 0 || ctrl[HD_N + 1] == 0)) return;
  const int bucket = LEVEL ? (int)ctrl[HD_SEL + 2 * (LEVEL - 1)] : 0;
  if (LEVEL == 2 && bucket == (int)ctrl[HD_SEL]) return;
  for (int k = threadIdx.x; k < HD_BINS; k += blockDim.x) h[k] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
    const int v = d2[i];
    const bool valid = v >= 0 && v < HD_LIMIT && (LEVEL == 0 || (v >> HD_SHIFT) == bucket);
    hd_hist_add(h, LEVEL ? (v & (HD_BINS - 1)) : (v >> HD_SHIFT), valid);
  }
  __syncthreads();
  unsigned* hist = ctrl + HD_CTRL + LEVEL * HD_BINS;
  for (int k = threadIdx.x; k < HD_BINS; k += blockDim.x)
    if (h[k]) atomicAdd(hist + k, h[k]);
}

// the bin that holds sorted rank r of a histogram (r < its total): the smallest b with hist[0] + .. + hist[b] > r, and r minus
// the counts below b.  One block of SURF_BLOCK threads, 32 bins each; sel[0..1] are written by the one thread whose range holds r.
__device__ void hd_select(const unsigned* __restrict__ hist, unsigned long long r, unsigned long long* part, unsigned* sel) {
  const int b0 = threadIdx.x * 32;
  unsigned long long s = 0;
  for (int b = b0; b < b0 + 32; ++b) s += hist[b];
  __syncthreads();
  part[threadIdx.x] = s;
  __syncthreads();
  unsigned long long acc = 0;
  for (int k = 0; k < (int)threadIdx.x; ++k) acc += part[k];
  if (r >= acc && r < acc + s) {
    for (int b = b0; b < b0 + 32; ++b) {
      const unsigned c = hist[b];
      if (r < acc + c) {
        sel[0] = (unsigned)b;
        sel[1] = (unsigned)(r - acc);
        break;
      }
      acc += c;
    }
  }
}

// after level 0: the gather blocks' partials to the label's counts and directed maxima, then the ranks
// lo = floor((n - 1) * quantile) (one fp64 product, rounded once) and hi = min(lo + 1, n - 1) of the pooled distances, each to
// its first-level bucket and its rank inside that bucket
__global__ __launch_bounds__(SURF_BLOCK) void hd_pick(unsigned* ctrl, const unsigned* __restrict__ gpart, int G, double quantile) {
  __shared__ unsigned long long part[SURF_BLOCK];
  __shared__ unsigned tot[4];
  if (threadIdx.x < 4) tot[threadIdx.x] = 0;
  __syncthreads();
  for (int dir = 0; dir < 2; ++dir) {
    unsigned nb = 0, mx = 0;
    for (int k = threadIdx.x; k < G; k += blockDim.x) {
      nb += gpart[2 * (dir * G + k)];
      mx = max(mx, gpart[2 * (dir * G + k) + 1]);
    }
    atomicAdd(&tot[HD_N + dir], nb);
    atomicMax(&tot[HD_MAX + dir], mx);
  }
  __syncthreads();
  if (threadIdx.x < 4) ctrl[threadIdx.x] = tot[threadIdx.x];
  if (tot[HD_N] == 0 || tot[HD_N + 1] == 0) return;
  const unsigned long long n = (unsigned long long)tot[HD_N] + tot[HD_N + 1];
  unsigned long long lo = (unsigned long long)floor(__dmul_rn((double)(n - 1), quantile));
  lo = lo < n - 1 ? lo : n - 1;
  const unsigned long long hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
  hd_select(ctrl + HD_CTRL, lo, part, ctrl + HD_SEL);
  hd_select(ctrl + HD_CTRL, hi, part, ctrl + HD_SEL + 2);
}

// out[l][6] = {border(P), border(G), max d^2 P -> G, max d^2 G -> P, d^2 at rank lo, d^2 at rank hi}; block l finishes label
// l + 1 from its second-level histograms
__global__ __launch_bounds__(SURF_BLOCK) void hd_final(const unsigned* __restrict__ ws, double* __restrict__ out) {
  __shared__ unsigned long long part[SURF_BLOCK];
  __shared__ unsigned bin[4];
  const unsigned* ctrl = ws + (int64_t)blockIdx.x * HD_LABEL_WORDS;
  double* o = out + 6 * (int64_t)blockIdx.x;
  const unsigned n_pg = ctrl[HD_N], n_gp = ctrl[HD_N + 1];
  if (n_pg == 0 || n_gp == 0) {
    if (threadIdx.x == 0) {
      o[0] = (double)n_pg;
      o[1] = (double)n_gp;
      for (int k = 2; k < 6; ++k) o[k] = -1.0;
    }
    return;
  }
  const unsigned b_lo = ctrl[HD_SEL], b_hi = ctrl[HD_SEL + 2];
  hd_select(ctrl + HD_CTRL + HD_BINS, ctrl[HD_SEL + 1], part, bin);
  hd_select(ctrl + HD_CTRL + (b_hi == b_lo ? 1 : 2) * HD_BINS, ctrl[HD_SEL + 3], part, bin + 2);
  __syncthreads();
  if (threadIdx.x == 0) {
    o[0] = (double)n_pg;
    o[1] = (double)n_gp;
    o[2] = (double)ctrl[HD_MAX];
    o[3] = (double)ctrl[HD_MAX + 1];
    o[4] = (double)((b_lo << HD_SHIFT) | bin[0]);
    o[5] = (double)((b_hi << HD_SHIFT) | bin[2]);
  }
}

struct HdLayout {
  int64_t part, d2, g, bytes;     // byte offsets; every label's control words and histograms come first
  int G;
};

HdLayout hd_layout(int D, int H, int W, int n_cls) {
  const int64_t N = (int64_t)D * H * W;
  HdLayout l;
  l.G = (int)std::min<int64_t>(cdiv64(N, SURF_BLOCK), SURF_GRID_CAP);
  l.part = cdiv64((int64_t)n_cls * HD_LABEL_WORDS * 4, 256) * 256;
  l.d2 = l.part + cdiv64((int64_t)2 * l.G * 2 * 4, 256) * 256;
  l.g = l.d2 + cdiv64(2 * N * 4, 256) * 256;
  l.bytes = l.g + N * 4;
  return l;
}

// ---------------------------------------------------------------------------------------------- anisotropic voxel spacing
// The same three passes with physical weights: squared distances are fp64, w = spacing^2 per axis (formed once on the host),
//   rows    wx * dx^2                        (the minimum over the integer dx^2 first: the product is monotone in it)
//   cols    min over y' of g(y') + wy * dy^2
//   gather  min over z' of g(z') + wz * dz^2
// dx^2, dy^2, dz^2 are integers below 2^24, converted exactly.  Every product is rounded on its own before it is added (the
// library is built with -ffp-contract=fast; sp_rounded is photo_rounded's trick from photometric.hip in fp64), so each value
// is one fixed expression of its inputs.  Two consequences the tests pin: with every weight 1 all values are the integers of
// the kernels above (sums below 2^26 are exact), and scaling all weights by a power of two scales every value by exactly it.
// "No feature" is +inf (a line without border voxels, the whole volume when the other mask is empty).
constexpr double SP_MIN = 1e-100, SP_MAX = 1e100;      // spacing range: s^2 .. 3 * 4095^2 * s^2 stay normal finite doubles

__device__ __forceinline__ double sp_rounded(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ double sp_inf() { return __longlong_as_double(0x7FF0000000000000LL); }

__global__ __launch_bounds__(SURF_BLOCK) void edt_rows_sp(const uint8_t* __restrict__ fb, int lab, double* __restrict__ g, int D,
                                                          int H, int W, int planar, double wx) {
  __shared__ int pos[SURF_MAX_DIM];
  __shared__ int npos;
  const int row = blockIdx.x;
  const int z = row / H, y = row % H;
  if (threadIdx.x == 0) npos = 0;
  __syncthreads();
  for (int x = threadIdx.x; x < W; x += blockDim.x)
    if (is_border(fb, lab, z, y, x, D, H, W, planar)) pos[atomicAdd(&npos, 1)] = x;
  __syncthreads();
  const int n = npos;
  double* out = g + (int64_t)row * W;
  for (int x = threadIdx.x; x < W; x += blockDim.x) {
    int best = SURF_INF;
    for (int k = 0; k < n; ++k) {
      const int d = x - pos[k];
      best = min(best, d * d);
    }
    out[x] = best < SURF_INF ? wx * (double)best : sp_inf();
  }
}

__global__ __launch_bounds__(SURF_BLOCK) void edt_cols_sp(double* g, int H, int W, double wy) {
  __shared__ double val[SURF_MAX_DIM];
  __shared__ int pos[SURF_MAX_DIM];
  __shared__ int npos;
  const int z = blockIdx.x / W, x = blockIdx.x % W;
  double* col = g + (int64_t)z * H * W + x;
  if (threadIdx.x == 0) npos = 0;
  __syncthreads();
  for (int y = threadIdx.x; y < H; y += blockDim.x) {
    const double v = col[(int64_t)y * W];
    if (v < sp_inf()) {
      const int k = atomicAdd(&npos, 1);
      val[k] = v;
      pos[k] = y;
    }
  }
  __syncthreads();
  const int n = npos;
  for (int y = threadIdx.x; y < H; y += blockDim.x) {
    double best = sp_inf();
    for (int k = 0; k < n; ++k) {
      const int d = y - pos[k];
      best = fmin(best, val[k] + sp_rounded(wy * (double)(d * d)));
    }
    col[(int64_t)y * W] = best;
  }
}

// the z pass at voxel (z, p) of the plane-major buffer g
__device__ __forceinline__ double sp_zmin(const double* __restrict__ g, int z, int64_t p, int D, int64_t HW, double wz) {
  double best = sp_inf();
  for (int zz = 0; zz < D; ++zz) {
    const int d = z - zz;
    best = fmin(best, g[zz * HW + p] + sp_rounded(wz * (double)(d * d)));
  }
  return best;
}

// edt_gather with weights.  A border voxel that has no feature at all (the other mask is empty) adds sqrt(SURF_INF), what it
// adds in edt_gather: the sum is as meaningless there as it is there, and the same number.
__global__ __launch_bounds__(SURF_BLOCK) void edt_gather_sp(const uint8_t* __restrict__ fa, int lab, const double* __restrict__ g,
                                                            double* __restrict__ part, int D, int H, int W, int planar,
                                                            double wz) {
  __shared__ double red[SURF_BLOCK / 64];
  const int64_t HW = (int64_t)H * W, N = HW * D;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double nb = 0.0, sum = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
    const int z = (int)(i / HW);
    const int64_t p = i - z * HW;
    const int y = (int)(p / W), x = (int)(p % W);
    if (!is_border(fa, lab, z, y, x, D, H, W, planar)) continue;
    const double best = sp_zmin(g, z, p, D, HW, wz);
    nb += 1.0;
    sum += sqrt(best < sp_inf() ? best : (double)SURF_INF);
  }
  nb = block_sum_d(nb, red);
  sum = block_sum_d(sum, red);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = nb;
    part[2 * blockIdx.x + 1] = sum;
  }
}

SurfLayout surf_layout_sp(int D, int H, int W, int n_cls) {
  SurfLayout l = surf_layout(D, H, W, n_cls);
  l.bytes = l.g + (int64_t)D * H * W * 8;
  return l;
}

bool spacing_ok(double s) { return s >= SP_MIN && s <= SP_MAX; }      // (false for NaN)

bool surf_sp_args_ok(int planar, double sz, double sy, double sx) {
  return (planar == 1 || spacing_ok(sz)) && spacing_ok(sy) && spacing_ok(sx);
}

// Hausdorff / percentile over fp64 squared distances.  A non-negative finite double orders as its bit pattern, so the key of
// a value is its 63-bit integer image (off the border the buffer holds -1.0: a negative key).  An MSD radix select takes the key
// of sorted rank lo in five levels of 13, 13, 13, 13 and 12 bits: level L histograms its digit over the entries whose higher
// bits equal the prefix chosen so far (LDS histogram per workgroup, flushed with integer atomicAdd), one block scans the 8192
// bins (hd_select above), extends the prefix and clears the bins for the next level.  After the last level the prefix IS the
// value at rank lo.  Rank hi = min(lo + 1, n - 1) holds the same value unless lo is the last entry of that value; then it is
// the smallest key above it, one integer atomicMin pass.  Only integer atomics: bitwise reproducible.  A label with an empty
// mask is known from the counts before the first level; every later kernel returns at once for it.
constexpr int SPH_LEVELS = 5;
constexpr int SPH_CTRL = 8;      // 64-bit control words of one label
enum { SPH_N = 0, SPH_MAX = 2, SPH_PREFIX = 4, SPH_RANK = 5, SPH_NEXT = 6, SPH_ABOVE = 7 };
// SPH_N: border voxels per direction; SPH_MAX: bits of the largest d^2 per direction; SPH_PREFIX: the key bits chosen so far;
// SPH_RANK: rank lo among the entries under the prefix; SPH_NEXT: before the last level 1 when hi = lo + 1, after it 1 when rank
// hi holds another value than rank lo; SPH_ABOVE: the smallest key above the value at rank lo

__host__ __device__ constexpr int sph_shift(int level) { return level < 4 ? 51 - 13 * level : 0; }      // 51, 38, 25, 12, 0
__host__ __device__ constexpr int sph_bits(int level) { return level < 4 ? 13 : 12; }

// edt_gather_d2 with weights: d2[i] = squared physical distance at the border voxels of `lab` in fa, -1.0 elsewhere;
// part[block] = {border voxels, max d^2}
__global__ __launch_bounds__(SURF_BLOCK) void edt_gather_d2_sp(const uint8_t* __restrict__ fa, int lab,
                                                               const double* __restrict__ g, double* __restrict__ d2,
                                                               double* __restrict__ part, int D, int H, int W, int planar,
                                                               double wz) {
  __shared__ double red[2 * (SURF_BLOCK / 64)];
  const int64_t HW = (int64_t)H * W, N = HW * D;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double nb = 0.0, mx = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
    const int z = (int)(i / HW);
    const int64_t p = i - z * HW;
    const int y = (int)(p / W), x = (int)(p % W);
    double v = -1.0;
    if (is_border(fa, lab, z, y, x, D, H, W, planar)) {
      v = sp_zmin(g, z, p, D, HW, wz);
      nb += 1.0;
      mx = fmax(mx, v);      // (+inf when the other mask is empty: hd_final_sp writes -1 then)
    }
    d2[i] = v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    nb += __shfl_xor(nb, o, 64);      // counts below 2^31: every partial sum is exact
    mx = fmax(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    red[2 * (threadIdx.x / 64)] = nb;
    red[2 * (threadIdx.x / 64) + 1] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < SURF_BLOCK / 64; ++k) {
      nb += red[2 * k];
      mx = fmax(mx, red[2 * k + 1]);
    }
    part[2 * blockIdx.x] = nb;
    part[2 * blockIdx.x + 1] = mx;
  }
}

// the gather blocks' partials to the label's counts and directed maxima, rank lo as in hd_pick, and the select's start state
__global__ __launch_bounds__(SURF_BLOCK) void hd_pick_sp(unsigned long long* ctrl, unsigned* hist, const double* __restrict__ gpart,
                                                         int G, double quantile) {
  __shared__ double s_nb[SURF_BLOCK], s_mx[SURF_BLOCK];
  for (int k = threadIdx.x; k < HD_BINS; k += blockDim.x) hist[k] = 0;
  double tot_n[2], tot_mx[2];
  for (int dir = 0; dir < 2; ++dir) {
    double nb = 0.0, mx = 0.0;
    for (int k = threadIdx.x; k < G; k += blockDim.x) {
      nb += gpart[2 * (dir * G + k)];
      mx = fmax(mx, gpart[2 * (dir * G + k) + 1]);
    }
    __syncthreads();
    s_nb[threadIdx.x] = nb;
    s_mx[threadIdx.x] = mx;
    __syncthreads();
    nb = 0.0, mx = 0.0;
    for (int k = 0; k < SURF_BLOCK; ++k) {
      nb += s_nb[k];
      mx = fmax(mx, s_mx[k]);
    }
    tot_n[dir] = nb;
    tot_mx[dir] = mx;
  }
  if (threadIdx.x != 0) return;
  const unsigned long long n_pg = (unsigned long long)tot_n[0], n_gp = (unsigned long long)tot_n[1];
  ctrl[SPH_N] = n_pg;
  ctrl[SPH_N + 1] = n_gp;
  ctrl[SPH_MAX] = (unsigned long long)__double_as_longlong(tot_mx[0]);
  ctrl[SPH_MAX + 1] = (unsigned long long)__double_as_longlong(tot_mx[1]);
  unsigned long long lo = 0, n = n_pg + n_gp;
  if (n_pg != 0 && n_gp != 0) {
    lo = (unsigned long long)floor(__dmul_rn((double)(n - 1), quantile));
    lo = lo < n - 1 ? lo : n - 1;
  }
  ctrl[SPH_PREFIX] = 0;
  ctrl[SPH_RANK] = lo;
  ctrl[SPH_NEXT] = (n_pg != 0 && n_gp != 0 && lo + 1 <= n - 1) ? 1 : 0;
  ctrl[SPH_ABOVE] = ~0ull;
}

template <int LEVEL>
__global__ __launch_bounds__(SURF_BLOCK) void hd_hist_sp(const long long* __restrict__ keys, int64_t n2,
                                                         const unsigned long long* __restrict__ ctrl, unsigned* hist) {
  __shared__ unsigned h[HD_BINS];
  if (ctrl[SPH_N] == 0 || ctrl[SPH_N + 1] == 0) return;
  constexpr int shift = sph_shift(LEVEL), bits = sph_bits(LEVEL);
  constexpr int above = LEVEL ? shift + bits : 63;      // level 0: nothing above but the sign, and the prefix is 0
  const long long prefix = (long long)ctrl[SPH_PREFIX];
  for (int k = threadIdx.x; k < HD_BINS; k += blockDim.x) h[k] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
    const long long v = keys[i];
    const bool valid = v >= 0 && (v >> above) == prefix;
    hd_hist_add(h, (int)((v >> shift) & ((1 << bits) - 1)), valid);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < HD_BINS; k += blockDim.x)
    if (h[k]) atomicAdd(hist + k, h[k]);
}

// one block: the bin of rank SPH_RANK in this level's histogram joins the prefix; the bins are cleared for the next level
template <int LEVEL>
__global__ __launch_bounds__(SURF_BLOCK) void hd_step_sp(unsigned long long* ctrl, unsigned* hist) {
  __shared__ unsigned long long part[SURF_BLOCK];
  __shared__ unsigned sel[2];
  if (ctrl[SPH_N] == 0 || ctrl[SPH_N + 1] == 0) return;
  hd_select(hist, ctrl[SPH_RANK], part, sel);
  __syncthreads();
  if (threadIdx.x == 0) {
    ctrl[SPH_PREFIX] = (ctrl[SPH_PREFIX] << sph_bits(LEVEL)) | sel[0];
    ctrl[SPH_RANK] = sel[1];
    if (LEVEL == SPH_LEVELS - 1) ctrl[SPH_NEXT] = (ctrl[SPH_NEXT] && sel[1] + 1 == hist[sel[0]]) ? 1 : 0;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < HD_BINS; k += blockDim.x) hist[k] = 0;
}

// the smallest key above the value at rank lo, only when rank hi needs it
__global__ __launch_bounds__(SURF_BLOCK) void hd_above_sp(const long long* __restrict__ keys, int64_t n2, unsigned long long* ctrl) {
  __shared__ unsigned long long m;
  if (ctrl[SPH_N] == 0 || ctrl[SPH_N + 1] == 0 || ctrl[SPH_NEXT] == 0) return;
  const long long v_lo = (long long)ctrl[SPH_PREFIX];
  if (threadIdx.x == 0) m = ~0ull;
  __syncthreads();
  unsigned long long best = ~0ull;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (int64_t)gridDim.x * blockDim.x) {
    const long long v = keys[i];
    if (v > v_lo) best = min(best, (unsigned long long)v);
  }
  if (best != ~0ull) atomicMin(&m, best);
  __syncthreads();
  if (threadIdx.x == 0 && m != ~0ull) atomicMin(ctrl + SPH_ABOVE, m);
}

// out[l][6] as hd_final, the four distance entries fp64 squared physical distances
__global__ void hd_final_sp(const unsigned long long* __restrict__ ws, double* __restrict__ out, int n_cls) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_cls) return;
  const unsigned long long* ctrl = ws + (int64_t)l * SPH_CTRL;
  double* o = out + 6 * (int64_t)l;
  o[0] = (double)ctrl[SPH_N];
  o[1] = (double)ctrl[SPH_N + 1];
  if (ctrl[SPH_N] == 0 || ctrl[SPH_N + 1] == 0) {
    for (int k = 2; k < 6; ++k) o[k] = -1.0;
    return;
  }
  o[2] = __longlong_as_double((long long)ctrl[SPH_MAX]);
  o[3] = __longlong_as_double((long long)ctrl[SPH_MAX + 1]);
  o[4] = __longlong_as_double((long long)ctrl[SPH_PREFIX]);
  o[5] = __longlong_as_double((long long)ctrl[ctrl[SPH_NEXT] ? SPH_ABOVE : SPH_PREFIX]);
}

struct HdSpLayout {
  int64_t hist, part, d2, g, bytes;     // byte offsets; every label's control words come first, then the one histogram
  int G;
};

HdSpLayout hd_layout_sp(int D, int H, int W, int n_cls) {
  const int64_t N = (int64_t)D * H * W;
  HdSpLayout l;
  l.G = (int)std::min<int64_t>(cdiv64(N, SURF_BLOCK), SURF_GRID_CAP);
  l.hist = cdiv64((int64_t)n_cls * SPH_CTRL * 8, 256) * 256;
  l.part = l.hist + (int64_t)HD_BINS * 4;
  l.d2 = l.part + cdiv64((int64_t)2 * l.G * 2 * 8, 256) * 256;
  l.g = l.d2 + cdiv64(2 * N * 8, 256) * 256;
  l.bytes = l.g + N * 8;
  return l;
}

template <int LEVEL>
void hd_level_sp(const long long* keys, int64_t n2, unsigned long long* ctrl, unsigned* hist, int hist_grid, hipStream_t s) {
  hd_hist_sp<LEVEL><<<hist_grid, SURF_BLOCK, 0, s>>>(keys, n2, ctrl, hist);
  hd_step_sp<LEVEL><<<1, SURF_BLOCK, 0, s>>>(ctrl, hist);
}

}  // namespace

extern "C" {

int64_t smsut_cc_ws(int D, int H, int W, int n_cls, int per_slice) {
  if (!cc_args_ok(D, H, W, n_cls, per_slice)) return -1;
  return cc_layout(D, H, W, n_cls, per_slice).bytes;
}

int smsut_cc_filter(const uint8_t* in, uint8_t* out, void* workspace, int D, int H, int W, int n_cls, int per_slice,
                    void* stream) {
  SMSUT_REQUIRE(in && out && workspace);
  SMSUT_REQUIRE(cc_args_ok(D, H, W, n_cls, per_slice));
  const CcLayout l = cc_layout(D, H, W, n_cls, per_slice);
  char* ws = (char*)workspace;
  int* err = (int*)ws;
  int* tot = (int*)(ws + l.tot);
  int* cnt = (int*)(ws + l.cnt);
  int* par = (int*)(ws + l.par);
  const int64_t N = (int64_t)D * H * W, HW = (int64_t)H * W;
  const int64_t ntot = (int64_t)(per_slice ? D : 1) * n_cls;
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = (unsigned)cdiv64(N, CC_BLOCK);
  cc_init<<<ew_grid(std::max(N, ntot), CC_BLOCK), CC_BLOCK, 0, s>>>(in, par, cnt, tot, err, N, ntot, n_cls);
  cc_merge<<<nb, CC_BLOCK, 0, s>>>(in, par, err, D, H, W, n_cls, per_slice);
  cc_count<<<nb, CC_BLOCK, 0, s>>>(in, par, cnt, tot, err, N, HW, n_cls, per_slice);
  cc_keep<<<nb, CC_BLOCK, 0, s>>>(in, out, par, cnt, tot, N, HW, n_cls, per_slice);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

int64_t smsut_surface_ws(int D, int H, int W, int n_cls, int planar) {
  if (!surf_args_ok(D, H, W, n_cls, planar)) return -1;
  return surf_layout(D, H, W, n_cls).bytes;
}

int smsut_surface_stats(const uint8_t* pred, const uint8_t* gt, double* out, void* workspace, int D, int H, int W, int n_cls,
                        int planar, void* stream) {
  SMSUT_REQUIRE(pred && gt && out && workspace);
  SMSUT_REQUIRE(surf_args_ok(D, H, W, n_cls, planar));
  const SurfLayout l = surf_layout(D, H, W, n_cls);
  char* ws = (char*)workspace;
  unsigned long long* cnt = (unsigned long long*)ws;
  double* part = (double*)(ws + l.part);
  int* g = (int*)(ws + l.g);
  const int64_t N = (int64_t)D * H * W;
  hipStream_t s = (hipStream_t)stream;
  surf_zero<<<1, SURF_BLOCK, 0, s>>>(cnt, 3 * n_cls);
  surf_counts<<<ew_grid(N, SURF_BLOCK), SURF_BLOCK, 0, s>>>(pred, gt, cnt, N, n_cls);
  for (int lab = 1; lab <= n_cls; ++lab) {
    for (int dir = 0; dir < 2; ++dir) {
      const uint8_t* fa = dir ? gt : pred;      // border voxels measured from ...
      const uint8_t* fb = dir ? pred : gt;      // ... to the border of the other mask
      edt_rows<<<(unsigned)(D * H), line_block(W), 0, s>>>(fb, lab, g, D, H, W, planar);
      edt_cols<<<(unsigned)(D * W), line_block(H), 0, s>>>(g, H, W);
      double* p = part + (int64_t)(2 * (lab - 1) + dir) * l.G * 2;
      edt_gather<<<l.G, SURF_BLOCK, 0, s>>>(fa, lab, g, p, D, H, W, planar);
    }
  }
  surf_final<<<2 * n_cls, SURF_BLOCK, 0, s>>>(cnt, part, out, l.G);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

int64_t smsut_surface_hd_ws(int D, int H, int W, int n_cls, int planar) {
  if (!surf_args_ok(D, H, W, n_cls, planar)) return -1;
  return hd_layout(D, H, W, n_cls).bytes;
}

int smsut_surface_hd(const uint8_t* pred, const uint8_t* gt, double* out, void* workspace, int D, int H, int W, int n_cls,
                     int planar, double quantile, void* stream) {
  SMSUT_REQUIRE(pred && gt && out && workspace);
  SMSUT_REQUIRE(surf_args_ok(D, H, W, n_cls, planar));
  SMSUT_REQUIRE(quantile > 0.0 && quantile <= 1.0);      // (false for NaN)
  const HdLayout l = hd_layout(D, H, W, n_cls);
  char* ws = (char*)workspace;
  unsigned* words = (unsigned*)ws;
  unsigned* part = (unsigned*)(ws + l.part);     // one label's gather partials at a time: hd_pick reads them before the next
  int* d2 = (int*)(ws + l.d2);
  int* g = (int*)(ws + l.g);
  const int64_t N = (int64_t)D * H * W;
  const int hist_grid = (int)std::min<int64_t>(cdiv64(2 * N, (int64_t)SURF_BLOCK * HD_HIST_ITEMS), HD_HIST_GRID_CAP);
  hipStream_t s = (hipStream_t)stream;
  hd_zero<<<ew_grid((int64_t)n_cls * HD_LABEL_WORDS, SURF_BLOCK), SURF_BLOCK, 0, s>>>(words, (int64_t)n_cls * HD_LABEL_WORDS);
  for (int lab = 1; lab <= n_cls; ++lab) {
    unsigned* ctrl = words + (int64_t)(lab - 1) * HD_LABEL_WORDS;
    for (int dir = 0; dir < 2; ++dir) {
      const uint8_t* fa = dir ? gt : pred;
      const uint8_t* fb = dir ? pred : gt;
      edt_rows<<<(unsigned)(D * H), line_block(W), 0, s>>>(fb, lab, g, D, H, W, planar);
      edt_cols<<<(unsigned)(D * W), line_block(H), 0, s>>>(g, H, W);
      edt_gather_d2<<<l.G, SURF_BLOCK, 0, s>>>(fa, lab, g, d2 + dir * N, part + (int64_t)dir * l.G * 2, D, H, W, planar);
    }
    hd_hist<0><<<hist_grid, SURF_BLOCK, 0, s>>>(d2, 2 * N, ctrl);
    hd_pick<<<1, SURF_BLOCK, 0, s>>>(ctrl, part, l.G, quantile);
    hd_hist<1><<<hist_grid, SURF_BLOCK, 0, s>>>(d2, 2 * N, ctrl);
    hd_hist<2><<<hist_grid, SURF_BLOCK, 0, s>>>(d2, 2 * N, ctrl);
  }
  hd_final<<<n_cls, SURF_BLOCK, 0, s>>>(words, out);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

int64_t smsut_surface_sp_ws(int D, int H, int W, int n_cls, int planar) {
  if (!surf_args_ok(D, H, W, n_cls, planar)) return -1;
  return surf_layout_sp(D, H, W, n_cls).bytes;
}

int smsut_surface_stats_sp(const uint8_t* pred, const uint8_t* gt, double* out, void* workspace, int D, int H, int W, int n_cls,
                           int planar, double sz, double sy, double sx, void* stream) {
  SMSUT_REQUIRE(pred && gt && out && workspace);
  SMSUT_REQUIRE(surf_args_ok(D, H, W, n_cls, planar));
  SMSUT_REQUIRE(surf_sp_args_ok(planar, sz, sy, sx));
  const SurfLayout l = surf_layout_sp(D, H, W, n_cls);
  char* ws = (char*)workspace;
  unsigned long long* cnt = (unsigned long long*)ws;
  double* part = (double*)(ws + l.part);
  double* g = (double*)(ws + l.g);
  const int64_t N = (int64_t)D * H * W;
  const double wz = planar ? 1.0 : sz * sz, wy = sy * sy, wx = sx * sx;
  hipStream_t s = (hipStream_t)stream;
  surf_zero<<<1, SURF_BLOCK, 0, s>>>(cnt, 3 * n_cls);
  surf_counts<<<ew_grid(N, SURF_BLOCK), SURF_BLOCK, 0, s>>>(pred, gt, cnt, N, n_cls);
  for (int lab = 1; lab <= n_cls; ++lab) {
    for (int dir = 0; dir < 2; ++dir) {
      const uint8_t* fa = dir ? gt : pred;
      const uint8_t* fb = dir ? pred : gt;
      edt_rows_sp<<<(unsigned)(D * H), line_block(W), 0, s>>>(fb, lab, g, D, H, W, planar, wx);
      edt_cols_sp<<<(unsigned)(D * W), line_block(H), 0, s>>>(g, H, W, wy);
      double* p = part + (int64_t)(2 * (lab - 1) + dir) * l.G * 2;
      edt_gather_sp<<<l.G, SURF_BLOCK, 0, s>>>(fa, lab, g, p, D, H, W, planar, wz);
    }
  }
  surf_final<<<2 * n_cls, SURF_BLOCK, 0, s>>>(cnt, part, out, l.G);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

int64_t smsut_surface_hd_sp_ws(int D, int H, int W, int n_cls, int planar) {
  if (!surf_args_ok(D, H, W, n_cls, planar)) return -1;
  return hd_layout_sp(D, H, W, n_cls).bytes;
}

int smsut_surface_hd_sp(const uint8_t* pred, const uint8_t* gt, double* out, void* workspace, int D, int H, int W, int n_cls,
                        int planar, double quantile, double sz, double sy, double sx, void* stream) {
  SMSUT_REQUIRE(pred && gt && out && workspace);
  SMSUT_REQUIRE(surf_args_ok(D, H, W, n_cls, planar));
  SMSUT_REQUIRE(quantile > 0.0 && quantile <= 1.0);      // (false for NaN)
  SMSUT_REQUIRE(surf_sp_args_ok(planar, sz, sy, sx));
  const HdSpLayout l = hd_layout_sp(D, H, W, n_cls);
  char* ws = (char*)workspace;
  unsigned long long* words = (unsigned long long*)ws;
  unsigned* hist = (unsigned*)(ws + l.hist);     // one histogram and one set of gather partials: the labels run one after another
  double* part = (double*)(ws + l.part);
  double* d2 = (double*)(ws + l.d2);
  double* g = (double*)(ws + l.g);
  const long long* keys = (const long long*)d2;
  const int64_t N = (int64_t)D * H * W;
  const double wz = planar ? 1.0 : sz * sz, wy = sy * sy, wx = sx * sx;
  const int hist_grid = (int)std::min<int64_t>(cdiv64(2 * N, (int64_t)SURF_BLOCK * HD_HIST_ITEMS), HD_HIST_GRID_CAP);
  hipStream_t s = (hipStream_t)stream;
  for (int lab = 1; lab <= n_cls; ++lab) {
    unsigned long long* ctrl = words + (int64_t)(lab - 1) * SPH_CTRL;
    for (int dir = 0; dir < 2; ++dir) {
      const uint8_t* fa = dir ? gt : pred;
      const uint8_t* fb = dir ? pred : gt;
      edt_rows_sp<<<(unsigned)(D * H), line_block(W), 0, s>>>(fb, lab, g, D, H, W, planar, wx);
      edt_cols_sp<<<(unsigned)(D * W), line_block(H), 0, s>>>(g, H, W, wy);
      edt_gather_d2_sp<<<l.G, SURF_BLOCK, 0, s>>>(fa, lab, g, d2 + dir * N, part + (int64_t)dir * l.G * 2, D, H, W, planar, wz);
    }
    hd_pick_sp<<<1, SURF_BLOCK, 0, s>>>(ctrl, hist, part, l.G, quantile);
    hd_level_sp<0>(keys, 2 * N, ctrl, hist, hist_grid, s);
    hd_level_sp<1>(keys, 2 * N, ctrl, hist, hist_grid, s);
    hd_level_sp<2>(keys, 2 * N, ctrl, hist, hist_grid, s);
    hd_level_sp<3>(keys, 2 * N, ctrl, hist, hist_grid, s);
    hd_level_sp<4>(keys, 2 * N, ctrl, hist, hist_grid, s);
    hd_above_sp<<<hist_grid, SURF_BLOCK, 0, s>>>(keys, 2 * N, ctrl);
  }
  hd_final_sp<<<(unsigned)cdiv64(n_cls, 64), 64, 0, s>>>(words, out, n_cls);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

}  // extern "C"
