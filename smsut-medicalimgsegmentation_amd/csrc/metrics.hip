// Test-phase metrics (reference misc/utils.py:18-36 connected_components, :206-283 get_all_matrix with medpy's dc / assd):
//   smsut_cc_filter      connected-component cleanup of every class 1..n_cls in one labelling pass (3-D 18-neighbour or
//                        per-slice 8-neighbour union-find, Playne & Hawick 2018), components of <= 10 % of their class dropped;
//   smsut_surface_stats  per label: Dice counts and, both ways, the border-voxel count and the fp64 sum of the exact Euclidean
//                        distances from one mask's border to the other's (separable squared EDT: brute-force minimum over each
//                        line's finite entries staged in LDS for x and y, the z pass fused with the gather).
// No float atomics: fp64 partials per block, reduced in a fixed order (bitwise reproducible).
#include <algorithm>

#include "common.h"
#include "smsut_hip.h"

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

}  // extern "C"
