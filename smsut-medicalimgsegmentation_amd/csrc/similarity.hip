// Translation metrics of the test phase (ops.image_similarity; misc/utils.py: TranslationMeter): per slice of two fp32 image
// batches a, b [N][H][W]
//   out[n][0] = sum over the (H-10)(W-10) window centres of SSIM(centre)     (Wang et al. 2004: 11x11 Gaussian window, sigma 1.5)
//   out[n][1] = SE = sum over ALL H W pixels of (a - b)^2
//   out[n][2] = AE = sum over ALL H W pixels of |a - b|
// One workgroup per TH x TW tile of window centres of ONE slice (blockIdx.y = n):
//   1. stage the tile and its 5-pixel halo of a and b in LDS, (TH+10) x (TW+10) dwords each, zero outside the image; the pixels
//      the tile OWNS (below) add their fp64 (a - b)^2 and |a - b| to the thread's SE / AE while they pass through registers;
//   2. horizontal pass: the 11 window weights over a, b, a^2, b^2, ab -> five LDS planes of (TH+10) x TW;
//   3. vertical pass: each thread slides down ROWS_PT consecutive centres of one column, every plane row read once per thread,
//      forms the fp32 SSIM of its centres and adds them in fp64;
//   4. fixed-order block sum of the three fp64 values -> ws[n][tile][3].
// A second launch (one workgroup per slice) adds a slice's tile partials in a fixed order and WRITES out[n][0..2].  No atomics, no
// tickets, no workgroup waits on another: the result is bitwise the same from call to call.  A slice's values never leave its
// own workgroups and its own row of ws / out, so a NaN or Inf stays in that slice's three outputs.
//
// LDS banks: in every pass a wave's 64 lanes are 64 consecutive columns of ONE row (reads and writes are 64 consecutive dwords:
// conflict-free for ds_read_b32 / ds_write_b32 whatever the row stride).  No lane group ever spans rows, so the plane stride TW = 64
// -- a multiple of 64 dwords, which would serialise a pass whose lanes walked DOWN a column -- costs nothing here.
//
// Window sums are fp32 in tap order k = 0 .. 10 (left to right, then top to bottom), the window weights 11 fp32 constants rounded
// once from the normalised fp64 Gaussian; the per-centre SSIM is fp32; every sum over centres or pixels is fp64.
#include <math.h>

#include "common.h"

namespace {
constexpr int TH = 32, TW = 64;              // tile of window centres (tests/ssim_ref.py names these two numbers)
constexpr int R = 5;                         // window radius
constexpr int SH = TH + 2 * R, SW = TW + 2 * R;   // staged rows / columns: 42 x 74
constexpr int TPB = 512;
constexpr int WAVES = TPB / 64;
constexpr int ROW_GROUPS = TPB / TW;         // 8 waves, one per group of ROWS_PT centre rows
constexpr int ROWS_PT = TH / ROW_GROUPS;     // 4 centres per thread in the vertical pass
static_assert(TW == 64 && TPB % TW == 0 && TH % ROW_GROUPS == 0, "a wave is one row of 64 columns in every pass");
constexpr int LDS_FLOATS = 2 * SH * SW + 5 * SH * TW;        // 6216 + 13440 floats = 78,624 bytes: two workgroups per CU
constexpr int MAX_HW = 4096, MAX_N = 65535;

// w[k] = exp(-(k-5)^2 / (2 * 1.5^2)) / sum, normalised in fp64, rounded once to fp32
__device__ constexpr float WGT[11] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,
                                      0x1.b43c4p-3f,   0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};

// The library is built with -ffp-contract=fast: the backend fuses x * y + z into an fma wherever it sees the pair, also through HIP's
// _rn intrinsics (plain operators) and under `#pragma clang fp contract(off)` (photometric.hip: photo_rounded).  Here that matters
// where a product meets a subtraction that cancels: s_a^2 = E[a^2] - mu_a^2 fused and s_ab = E[ab] - mu_a mu_b not (the choice is
// the optimiser's, per expression) differ by the rounding of a product, ~3e-8, next to C2 = 9e-4 -- 6e-5 in a constant image's SSIM.
// A product passed through an empty asm statement is rounded as written: no instruction, and nothing left to fuse.
__device__ __forceinline__ float rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ double rounded(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

// fixed-order sum of three doubles over a TPB-thread block -> thread 0; sm: 3 * WAVES doubles
__device__ __forceinline__ void block_sum3(double (&v)[3], double* sm) {
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = wave_sum_d(v[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) sm[(threadIdx.x >> 6) * 3 + k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double t = 0.0;
      for (int w = 0; w < WAVES; ++w) t += sm[w * 3 + k];
      v[k] = t;
    }
  }
}

__global__ void __launch_bounds__(TPB)
k_similarity_tiles(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ part, int H, int W, int tiles_x,
                   int tiles_y, float c1, float c2) {
  __shared__ float lds[LDS_FLOATS];
  __shared__ double red[3 * WAVES];
  float* sa = lds;                           // [SH][SW]
  float* sb = lds + SH * SW;
  float* pl = lds + 2 * SH * SW;             // [5][SH][TW]: a, b, a^2, b^2, ab after the horizontal pass
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, n = blockIdx.y;
  const int x0 = tx * TW, y0 = ty * TH;      // first staged pixel = first centre of the tile minus the radius
  const int cw = min(TW, W - 2 * R - x0), ch = min(TH, H - 2 * R - y0);     // centres of this tile: >= 1 each
  // OWNERSHIP of pixels (SE, AE): a pixel belongs to the tile whose centres hold its coordinates, and the 5-pixel frame of the
  // image, which holds no centre, to the edge tiles next to it.  Rows [oy0, oy1), columns [ox0, ox1): the tiles' rectangles
  // partition [0, H) x [0, W), and each lies inside its tile's staged block [y0, y0 + SH) x [x0, x0 + SW) -- for the last tile
  // because its centres end at H - 6, so H <= y0 + ch + 10 <= y0 + SH.
  const int oy0 = ty == 0 ? 0 : y0 + R, oy1 = ty == tiles_y - 1 ? H : y0 + R + TH;
  const int ox0 = tx == 0 ? 0 : x0 + R, ox1 = tx == tiles_x - 1 ? W : x0 + R + TW;
  const size_t base = (size_t)n * H * W;
  double acc[3] = {0.0, 0.0, 0.0};           // {sum of SSIM, SE, AE} of this thread

  // ---- 1. stage (dword loads: a slice starts anywhere, H W need not be a multiple of 4) ----
  for (int i = threadIdx.x; i < SH * SW; i += TPB) {
    const int r = i / SW, c = i - r * SW;
    const int y = y0 + r, x = x0 + c;
    float va = 0.f, vb = 0.f;
    if (y < H && x < W) {
      const size_t g = base + (size_t)y * W + x;
      va = a[g]; vb = b[g];
      if (y >= oy0 && y < oy1 && x >= ox0 && x < ox1) {
        const double d = (double)va - (double)vb;
        acc[1] += rounded(d * d);            // (the square rounded as the product it is defined as, not fused into the add)
        acc[2] += fabs(d);
      }
    }
    sa[i] = va; sb[i] = vb;
  }
  __syncthreads();

  // ---- 2. horizontal pass: thread = (row group, column); taps left to right ----
  const int col = threadIdx.x & (TW - 1), grp = threadIdx.x / TW;
  for (int r = grp; r < SH; r += ROW_GROUPS) {
    const float* ra = sa + r * SW + col;
    const float* rb = sb + r * SW + col;
    float ma = 0.f, mb = 0.f, maa = 0.f, mbb = 0.f, mab = 0.f;
#pragma unroll
    for (int k = 0; k < 2 * R + 1; ++k) {
      const float va = ra[k], vb = rb[k], w = WGT[k];
      // (each square / product rounded once -- an fma operand, nothing to fuse it with -- and each tap ONE fma, written out: the
      //  same sequence for all five planes, so that a == b makes the a^2, b^2 and ab planes bitwise equal)
      const float aa = va * va, bb = vb * vb, ab = va * vb;
      ma = __fmaf_rn(w, va, ma); mb = __fmaf_rn(w, vb, mb);
      maa = __fmaf_rn(w, aa, maa); mbb = __fmaf_rn(w, bb, mbb); mab = __fmaf_rn(w, ab, mab);
    }
    float* o = pl + r * TW + col;
    o[0] = ma; o[SH * TW] = mb; o[2 * SH * TW] = maa; o[3 * SH * TW] = mbb; o[4 * SH * TW] = mab;
  }
  __syncthreads();

  // ---- 3. vertical pass: thread = column `col`, centres rows grp * ROWS_PT .. + ROWS_PT - 1; taps top to bottom ----
  if (grp * ROWS_PT < ch) {                  // (wave-uniform)
    float s[ROWS_PT][5];
#pragma unroll
    for (int o = 0; o < ROWS_PT; ++o)
#pragma unroll
      for (int q = 0; q < 5; ++q) s[o][q] = 0.f;
    const float* p0 = pl + (grp * ROWS_PT) * TW + col;
#pragma unroll
    for (int r = 0; r < ROWS_PT + 2 * R; ++r) {          // plane row grp * ROWS_PT + r <= SH - 1
      float v[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) v[q] = p0[q * SH * TW + r * TW];
#pragma unroll
      for (int o = 0; o < ROWS_PT; ++o) {
        if (r - o >= 0 && r - o <= 2 * R) {              // (compile time) row r is tap r - o of centre o
#pragma unroll
          for (int q = 0; q < 5; ++q) s[o][q] = __fmaf_rn(WGT[r - o], v[q], s[o][q]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < ROWS_PT; ++o) {
      // the three products of means rounded as written (`rounded`, above), every other step a sum or a product of sums: with a == b
      // the numerator and the denominator are then the same fp32 numbers term by term -- 2 rn(mx my) = rn(mx^2) + rn(my^2),
      // 2 sxy = sx + sy -- and the value is exactly 1
      const float mx = s[o][0], my = s[o][1];
      const float mxx = rounded(mx * mx), myy = rounded(my * my), mxy = rounded(mx * my);
      const float sx = s[o][2] - mxx, sy = s[o][3] - myy, sxy = s[o][4] - mxy;
      const float num = (2.f * mxy + c1) * (2.f * sxy + c2);
      const float den = ((mxx + myy) + c1) * ((sx + sy) + c2);
      const float v = num / den;
      if (grp * ROWS_PT + o < ch && col < cw) acc[0] += (double)v;
    }
  }

  // ---- 4. the workgroup's three sums, in a fixed order ----
  block_sum3(acc, red);
  if (threadIdx.x == 0) {
    double* o = part + ((size_t)n * gridDim.x + blockIdx.x) * 3;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
  }
}

// out[n][k] = sum over the slice's tiles of part[n][tile][k]: thread t adds tiles t, t + TPB, ... in order, then the block sum
__global__ void __launch_bounds__(TPB)
k_similarity_final(const double* __restrict__ part, double* __restrict__ out, int tiles) {
  __shared__ double red[3 * WAVES];
  const int n = blockIdx.x;
  const double* p = part + (size_t)n * tiles * 3;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int t = threadIdx.x; t < tiles; t += TPB) {
    acc[0] += p[t * 3]; acc[1] += p[t * 3 + 1]; acc[2] += p[t * 3 + 2];
  }
  block_sum3(acc, red);
  if (threadIdx.x == 0) { out[n * 3] = acc[0]; out[n * 3 + 1] = acc[1]; out[n * 3 + 2] = acc[2]; }
}

inline bool dims_ok(int n, int h, int w) {
  return n >= 1 && n <= MAX_N && h >= 2 * R + 1 && h <= MAX_HW && w >= 2 * R + 1 && w <= MAX_HW;
}
inline int tiles_along(int len, int tile) { return (len - 2 * R + tile - 1) / tile; }

}  // namespace

extern "C" {

int64_t smsut_image_similarity_ws(int n, int h, int w) {
  if (!dims_ok(n, h, w)) return -1;
  return (int64_t)n * tiles_along(h, TH) * tiles_along(w, TW) * 3 * (int64_t)sizeof(double);
}

int smsut_image_similarity(const float* a, const float* b, double* out, void* ws, int n, int h, int w, double data_range,
                           void* stream) {
  SMSUT_REQUIRE(dims_ok(n, h, w));
  SMSUT_REQUIRE(isfinite(data_range) && data_range > 0.0);
  SMSUT_REQUIRE(a && b && out && ws);
  const int tiles_x = tiles_along(w, TW), tiles_y = tiles_along(h, TH);      // <= 64 x 128
  const float c1 = (float)((0.01 * data_range) * (0.01 * data_range)), c2 = (float)((0.03 * data_range) * (0.03 * data_range));
  k_similarity_tiles<<<dim3((unsigned)(tiles_x * tiles_y), (unsigned)n), TPB, 0, (hipStream_t)stream>>>(
      a, b, (double*)ws, h, w, tiles_x, tiles_y, c1, c2);
  SMSUT_LAUNCH_CHECK();
  k_similarity_final<<<(unsigned)n, TPB, 0, (hipStream_t)stream>>>((const double*)ws, out, tiles_x * tiles_y);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

}  // extern "C"
