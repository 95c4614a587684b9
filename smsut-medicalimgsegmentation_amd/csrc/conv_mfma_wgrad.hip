// LDS-staged weight gradient of the MFMA convolutions (fp32 v_mfma_f32_16x16x4_f32, or fp16 operands; fp32 accumulate):
//
//   gW[tap][k][n] = sum_p in[p + off(tap), k] * gy[p, n]   (GEMM with the pixels as K)
//
// for the 3x3 / 1x1 "same" convs, the 4x4 stride-1 pad-1 conv and ConvTranspose2x2.  The forward / data-gradient family is
// conv_mfma.hip, the register-row kernel (first rung of the ladder wgrad_select walks) conv_wgrad_rr.hip; conv_mfma.h holds the
// device primitives shared with the forward file.
//
// Weight-grad tiling: a workgroup owns a (16*CIT x 16*COT) slab of gW for all taps and walks a range of
// 8x16-pixel tiles; the 4 waves split each tile's rows (the GEMM K dimension), keep taps*CIT*COT
// accumulators in registers across all its tiles, and are combined once at the end through LDS in a fixed
// order; per-split slabs are summed by a second tiny kernel (deterministic, no atomics).
#include "conv_mfma.h"
#include "conv_wgrad_rr.h"

namespace {

// conv_f16_wgrad: the transposing LDS read's result type, and the 16- / 32-deep MFMA (conv_mfma.h) picked by the operand width
typedef short s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfmak(h4 a, h4 b, f32x4 c) { return mfma16h(a, b, c); }
__device__ __forceinline__ f32x4 mfmak(h8 a, h8 b, f32x4 c) { return mfma32h(a, b, c); }

// ------------------------------------------------------------------------------------------------ weight gradient
constexpr int WTH = 8;       // pixel tile rows; each wave takes WTH/4 = 2 rows (the GEMM K dimension)
#ifndef WG_RR_UNROLL
#define WG_RR_UNROLL 2
#endif
#ifndef WG_KS_UNROLL
#define WG_KS_UNROLL 4
#endif
#ifndef WG11_MIN_BLOCKS
#define WG11_MIN_BLOCKS 1    // 16x16-slab weight gradient: workgroups per CU the register allocation must allow (r02 A/B on
                             // H256 16->16 B32: uncapped 168 VGPR / 3 waves 104 us; cap 4 with the row loop rolled (94-111 VGPR)
                             // 103-126 us; cap 4 fully unrolled spills -- occupancy is not what limits this kernel)
#endif
// WTS_ROLL (r03): lane (channel lm, k-slot kq) of the tap-split weight gradient covers FOUR CONSECUTIVE pixels 4kq .. 4kq+3 of a
// tile row (MFMA ks takes pixel 4kq + ks) instead of the pixels kq, 4 + kq, ...: the three horizontal taps of its four pixels are
// then the six pixels 4kq .. 4kq+5 of the haloed row -- six registers instead of twelve LDS reads -- and the three rows a tile
// row needs roll through registers, ONE new row per tile row: 10 LDS reads per 36 MFMAs instead of 40.  The k-slot stride in LDS
// becomes 4 pixels, so the pixel stride is 36 floats (4 x 36 = 16 mod 64 banks: the four k-slots of a read on disjoint bank
// quarters; with the old stride of 48 they would collide four ways), 68 for the [gy | gs] tile of the fused-shortcut form.
#ifndef WTS_STRIDE_VALUE
#define WTS_STRIDE_VALUE 36
#endif
constexpr int WTS_STRIDE_SC = 68;   // ... of the fused-shortcut form's [gy 32 | gs 32 | pad] tile
constexpr int WTS_STRIDE = WTS_STRIDE_VALUE;   // pixel stride (floats) of the tap-split wgrad's LDS tiles (32 channels + pad)

template <int KS, int CIT, int COT, bool DUAL = false, bool INAFF = false, bool C8 = false, bool SC8 = false>
__global__ void __launch_bounds__(TPB, (KS == 3 && CIT == 1 && COT == 1 && !INAFF) ? WG11_MIN_BLOCKS : 1)
conv_mfma_wgrad(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ part, int N, int H,
                int W, int Cin, int Cout, int tiles_x, int tiles_y, int tiles_per_split, int gsc, int nci,
                const float* __restrict__ x2 = nullptr, int ca = 0, AffRef aff = AffRef{},
                const float* __restrict__ gs = nullptr) {
  // SC8 (with C8): the weight gradient of the first block's 1x1 shortcut rides along (see conv_mfma_wgrad_ts, SC): one more
  // accumulator tile = the (tap 4 | tap 5) group's x rows against gs; rows 0-7 (tap 4 = the centre) are the shortcut's gradient,
  // written as slab row KK of a (KK+1)-row slab; rows 8-15 are discarded.
  static_assert(!SC8 || C8, "fused shortcut weight gradient of the 8-channel form");
  // INAFF: x is the raw conv output whose lrelu(IN(.)) is the operand (see AffRef); applied when a tile is published.
  // gsc = 2 / 4 tap groups in blockIdx.y: weight-gradient of ConvTranspose2x2 (gy is the 2x larger tensor).
  // C8: Cin == 8 (first block after the stem).  Half of the 16 MFMA rows would be padding; instead PAIRS OF TAPS share one
  // accumulator tile: rows 0-7 = (tap 2g, ci), rows 8-15 = (tap 2g+1, ci) -- lane lm reads x at its tap's halo offset --
  // 5 accumulator tiles and 5 MFMAs per pixel quad instead of 9.
  static_assert(!C8 || (KS == 3 && CIT == 1 && !DUAL && !INAFF), "8-channel form: plain 3x3");
  constexpr int KK = KS * KS;
  constexpr int PAD = (KS - 1) / 2;
  constexpr int IH = WTH + KS - 1, IW = TW + KS - 1;
  constexpr int CI_T = 16 * CIT, CO_T = 16 * COT;
  constexpr int SI = (CI_T % 32 == 16) ? CI_T : CI_T + 16;     // pixel stride = 16 (mod 32): 4 pixels x 16 ch conflict-free
  constexpr int SO = (CO_T % 32 == 16) ? CO_T : CO_T + 16;
  constexpr int NG = C8 ? (KK + 1) / 2 : KK;   // accumulator tile groups per (ci tile, co tile): taps, or tap pairs
  constexpr int NACC = (NG + (SC8 ? 1 : 0)) * CIT * COT;
  extern __shared__ float smem[];
  float* in_s = smem;                         // [IH][IW][SI]
  float* gy_s = smem + IH * IW * SI;          // [WTH][TW][SO]
  [[maybe_unused]] float* gs_s = gy_s + WTH * TW * SO;   // SC8: [WTH][TW][SO]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, kq = lane >> 4;
  const int split = blockIdx.x;
  const int tg = blockIdx.y / nci;
  const int ci0 = (blockIdx.y % nci) * CI_T, co0 = blockIdx.z * CO_T;
  const int Wg = W * gsc;
  const int tiles_img = tiles_x * tiles_y;
  const int total_tiles = N * tiles_img;
  const int t_begin = split * tiles_per_split;
  const int t_end = min(t_begin + tiles_per_split, total_tiles);

  f32x4 acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  constexpr int NIN = (IH * IW * (CI_T / 4) + TPB - 1) / TPB;
  constexpr int NGY = (WTH * TW * (CO_T / 4) + TPB - 1) / TPB;
  float4 rin[NIN], rgy[NGY];
  [[maybe_unused]] float4 rgs[NGY];
  // per-thread unit descriptors, computed once: (iy << 8 | ix) inside the tile, or -1; channel of the unit
  int in_yx[NIN], in_c[NIN], in_lds[NIN], gy_yx[NGY], gy_c[NGY], gy_lds[NGY];
#pragma unroll
  for (int i = 0; i < NIN; ++i) {
    const int u = tid + i * TPB;
    const int q = u % (CI_T / 4), pix = u / (CI_T / 4);
    const int c = ci0 + 4 * q;
    in_yx[i] = (u < IH * IW * (CI_T / 4) && c < Cin) ? (((pix / IW) << 8) | (pix % IW)) : -1;
    in_c[i] = c;
    in_lds[i] = pix * SI + 4 * q;
  }
#pragma unroll
  for (int i = 0; i < NGY; ++i) {
    const int u = tid + i * TPB;
    const int q = u % (CO_T / 4), pix = u / (CO_T / 4);
    const int c = co0 + 4 * q;
    gy_yx[i] = (u < WTH * TW * (CO_T / 4) && c < Cout) ? (((pix / TW) << 8) | (pix % TW)) : -1;
    gy_c[i] = c;
    gy_lds[i] = pix * SO + 4 * q;
  }

  // DUAL: x is the virtual cat([x, x2]); a thread's units share one channel quad (see conv_mfma_wgrad_ts).  A template
  // flag, so the plain form keeps its uniform (scalar-register) base and stride: a runtime select cost it 15 % at 16->16.
  const CatSrc xsrc = DUAL ? cat_src(x, x2, Cin, ca, ci0 + 4 * (tid % (CI_T / 4))) : CatSrc{x, Cin, 0};
  [[maybe_unused]] unsigned inimg = 0;                          // INAFF: units of rin that lie inside the image
  [[maybe_unused]] float4 a_m, a_r, a_g, a_b;
  [[maybe_unused]] const int aq = ci0 + 4 * (tid % (CI_T / 4));   // this thread's channel quad (same for all its units)
  if (INAFF) {
    a_g = a_b = make_float4(0.f, 0.f, 0.f, 0.f);
    if (aq < Cin) { a_g = *(const float4*)(aff.gamma + aq); a_b = *(const float4*)(aff.beta + aq); }
  }
  auto prefetch = [&](int t) {
    const int n_img = t / tiles_img;
    const int rem = t % tiles_img;
    const int y0 = (rem / tiles_x) * WTH, x0 = (rem % tiles_x) * TW;
    const float* xin = xsrc.p + (size_t)n_img * H * W * xsrc.stride - xsrc.coff;
    const float* gin = gy + (size_t)n_img * H * gsc * Wg * Cout;
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int gy_ = y0 + (in_yx[i] >> 8) - PAD, gx_ = x0 + (in_yx[i] & 255) - PAD;
      if (in_yx[i] >= 0 && gy_ >= 0 && gy_ < H && gx_ >= 0 && gx_ < W) {
        v = *(const float4*)(xin + ((size_t)gy_ * W + gx_) * xsrc.stride + in_c[i]);
        if (INAFF) inimg |= 1u << i;
      } else if (INAFF) inimg &= ~(1u << i);
      rin[i] = v;
    }
    if (INAFF && aq < Cin) {
      a_m = *(const float4*)(aff.mean + (size_t)n_img * Cin + aq);
      a_r = *(const float4*)(aff.rstd + (size_t)n_img * Cin + aq);
    }
#pragma unroll
    for (int i = 0; i < NGY; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int gy_ = y0 + (gy_yx[i] >> 8), gx_ = x0 + (gy_yx[i] & 255);
      if (gy_yx[i] >= 0 && gy_ < H && gx_ < W)
        v = *(const float4*)(gin + ((size_t)(gy_ * gsc + (tg >> 1)) * Wg + gx_ * gsc + (tg & 1)) * Cout + gy_c[i]);
      rgy[i] = v;
      if constexpr (SC8) {                     // (gsc == 1: same geometry as gy)
        float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gy_yx[i] >= 0 && gy_ < H && gx_ < W)
          u = *(const float4*)(gs + (size_t)n_img * H * W * Cout + ((size_t)gy_ * W + gx_) * Cout + gy_c[i]);
        rgs[i] = u;
      }
    }
  };

  if (t_begin < t_end) prefetch(t_begin);
  for (int t = t_begin; t < t_end; ++t) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NIN; ++i)
      if (tid + i * TPB < IH * IW * (CI_T / 4)) {
        float4 v = rin[i];
        if (INAFF && ((inimg >> i) & 1u)) {
          v.x = aff1(v.x, a_m.x, a_r.x, a_g.x, a_b.x, aff.slope); v.y = aff1(v.y, a_m.y, a_r.y, a_g.y, a_b.y, aff.slope);
          v.z = aff1(v.z, a_m.z, a_r.z, a_g.z, a_b.z, aff.slope); v.w = aff1(v.w, a_m.w, a_r.w, a_g.w, a_b.w, aff.slope);
        }
        *(float4*)(in_s + in_lds[i]) = v;
      }
#pragma unroll
    for (int i = 0; i < NGY; ++i)
      if (tid + i * TPB < WTH * TW * (CO_T / 4)) {
        *(float4*)(gy_s + gy_lds[i]) = rgy[i];
        if constexpr (SC8) *(float4*)(gs_s + gy_lds[i]) = rgs[i];
      }
    __syncthreads();
    if (t + 1 < t_end) prefetch(t + 1);
#pragma unroll WG_RR_UNROLL
    for (int rr = 0; rr < WTH / 4; ++rr) {
      const int r = wave * (WTH / 4) + rr;
#pragma unroll WG_KS_UNROLL
      for (int ks = 0; ks < TW / 4; ++ks) {
        const int px = ks * 4 + kq;                 // this lane's pixel (the MFMA k index) within the row
        float b[COT];
#pragma unroll
        for (int j = 0; j < COT; ++j) b[j] = gy_s[(r * TW + px) * SO + j * 16 + lm];
        if constexpr (C8) {
          const int hi = lm >> 3;                    // this lane's MFMA row belongs to the second tap of the pair
#pragma unroll
          for (int g = 0; g < NG; ++g) {
            const int tB = (2 * g + 1 < KK) ? 2 * g + 1 : 2 * g;
            const int t = hi ? tB : 2 * g;
            float a = in_s[((r + t / KS) * IW + px + t % KS) * SI + (lm & 7)];
            if (hi && 2 * g + 1 >= KK) a = 0.f;      // the unpaired last tap
#pragma unroll
            for (int j = 0; j < COT; ++j) acc[g * COT + j] = mfma16(a, b[j], acc[g * COT + j]);
            if constexpr (SC8) {
              if (2 * g == KK / 2) {                 // rows 0-7 of this group are the centre tap
#pragma unroll
                for (int j = 0; j < COT; ++j)
                  acc[NG * COT + j] = mfma16(a, gs_s[(r * TW + px) * SO + j * 16 + lm], acc[NG * COT + j]);
              }
            }
          }
        } else
#pragma unroll
        for (int tap = 0; tap < KK; ++tap) {
          const int kh = tap / KS, kw = tap % KS;
#pragma unroll
          for (int i = 0; i < CIT; ++i) {
            const float a = in_s[((r + kh) * IW + px + kw) * SI + i * 16 + lm];
#pragma unroll
            for (int j = 0; j < COT; ++j)
              acc[(tap * CIT + i) * COT + j] = mfma16(a, b[j], acc[(tap * CIT + i) * COT + j]);
          }
        }
      }
    }
  }
  // ---- combine the 4 waves in a fixed order (wave 0 += wave 1, 2, 3) through LDS, then wave 0 stores the slab
  float* red = smem;      // NACC * 64 * 4 floats
  for (int src = 1; src < 4; ++src) {
    __syncthreads();
    if (wave == src) {
#pragma unroll
      for (int i = 0; i < NACC; ++i) *(f32x4*)(red + ((size_t)i * 64 + lane) * 4) = acc[i];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int i = 0; i < NACC; ++i) acc[i] += *(const f32x4*)(red + ((size_t)i * 64 + lane) * 4);
    }
  }
  if (C8) {
    if (wave == 0) {
      float* out = part + (size_t)split * (SC8 ? KK + 1 : KK) * Cin * Cout;   // rows 4kq + r: tap 2g + (row >> 3), ci = row & 7
      if constexpr (SC8) {
#pragma unroll
        for (int j = 0; j < COT; ++j) {
          const int co = co0 + j * 16 + lm;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 4 * kq + r;
            if (row < 8 && co < Cout) out[((size_t)KK * Cin + row) * Cout + co] = acc[NG * COT + j][r];
          }
        }
      }
#pragma unroll
      for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int j = 0; j < COT; ++j) {
          const int co = co0 + j * 16 + lm;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = 4 * kq + r, tap = 2 * g + (row >> 3);
            if (tap < KK && co < Cout) out[((size_t)tap * Cin + (row & 7)) * Cout + co] = acc[g * COT + j][r];
          }
        }
    }
    return;
  }
  if (wave == 0) {
    float* out = part + ((size_t)split * (gridDim.y / nci) + tg) * KK * Cin * Cout;
#pragma unroll
    for (int tap = 0; tap < KK; ++tap)
#pragma unroll
      for (int i = 0; i < CIT; ++i)
#pragma unroll
        for (int j = 0; j < COT; ++j) {
          const int co = co0 + j * 16 + lm;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ci = ci0 + i * 16 + 4 * kq + r;
            if (ci < Cin && co < Cout) out[((size_t)tap * Cin + ci) * Cout + co] = acc[(tap * CIT + i) * COT + j][r];
          }
        }
  }
}

// Tap-split weight gradient for the 32x32-channel slab (KS = 3): the 36 accumulator tiles (tap, ci-tile, co-tile) are
// dealt round-robin to the 4 waves -- 9 each -- and every wave walks ALL pixels of the staged tile.  Compared with the
// row-split kernel above (each wave 1/4 of the rows, all 36 tiles = 144 accumulator registers, one wave per SIMD,
// three LDS combine rounds at the end) this needs 36 accumulator registers, keeps two workgroups per CU resident and
// has no cross-wave combine: each wave stores its own tiles.  PMC r01 (64->64 @64^2): row-split 46 % MFMA busy.
typedef f32x4 wvec;
#define WZERO ((f32x4){0.f, 0.f, 0.f, 0.f})
template <bool DUAL = false, bool INAFF = false, bool SC = false>
__global__ void __launch_bounds__(TPB)
conv_mfma_wgrad_ts(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ part, int N, int H,
                   int W, int Cin, int Cout, int tiles_x, int tiles_y, int tiles_per_split,
                   const float* __restrict__ x2 = nullptr, int ca = 0, AffRef aff = AffRef{},
                   const float* __restrict__ gs = nullptr) {
  // SC: the weight gradient of the block's 1x1 shortcut conv rides along (network/blocks.py:66-80: conv1 and the shortcut read
  // the same x): a tenth "tap" whose A operand is the centre tap's x and whose B operand is gs (the gradient of the shortcut's
  // output) -- every wave gets ONE more accumulator tile (ci tile wave >> 1, its co tile), stored as row KK of a (KK+1)-row slab.  gy and gs share one LDS tile [pixel][gy 32 | gs 32 | pad 16]
  // (80-float stride: pixel groups kq, kq + 1 still land on disjoint bank halves), 75.5 KB with the x tile: two workgroups per CU.
  static_assert(!SC || !INAFF, "fused shortcut weight gradient: plain / virtual-cat input");
  constexpr int KS = 3, KK = 9, PAD = 1, CIT = 2, COT = 2;
  constexpr int IH = WTH + KS - 1, IW = TW + KS - 1;
  constexpr int CI_T = 32, CO_T = 32, SI = WTS_STRIDE, SO = SC ? WTS_STRIDE_SC : WTS_STRIDE;
  constexpr int NSLOT = KK * CIT * COT / 4;                    // 9 accumulator tiles per wave
  extern __shared__ float smem[];
  float* in_s = smem;                         // [IH][IW][SI]
  float* gy_s = smem + IH * IW * SI;          // [WTH][TW][SO]
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, kq = lane >> 4;
  const int split = blockIdx.x;
  const int ci0 = blockIdx.y * CI_T, co0 = blockIdx.z * CO_T;
  const int tiles_img = tiles_x * tiles_y;
  const int total_tiles = N * tiles_img;
  const int t_begin = split * tiles_per_split;
  const int t_end = min(t_begin + tiles_per_split, total_tiles);

  // this wave's unit k is tap k of ci tile wave >> 1 against co tile wave & 1
  const int jt = wave & 1;
  f32x4 acc[NSLOT];
#pragma unroll
  for (int k = 0; k < NSLOT; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
  [[maybe_unused]] f32x4 acc_sc = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Staging descriptors, computed once (full tiles and full 32-channel slabs only -- the host checks H % 8 == 0,
  // W % 16 == 0, Cin % 32 == 0, Cout % 32 == 0 and 32-bit element offsets): element offset of the unit relative to the
  // tile's first halo pixel, LDS slot (a dummy slot for the padding units), image borders the unit falls outside of.
  constexpr int UIN = IH * IW * (CI_T / 4);
  constexpr int NIN = (UIN + TPB - 1) / TPB;
  constexpr int NGY = (WTH * TW * (CO_T / 4) + TPB - 1) / TPB;
  static_assert(WTH * TW * (CO_T / 4) % TPB == 0, "gy tile units divide evenly");
  wvec rin[NIN], rgy[NGY];     // ext-vector values (HIP's float4 struct kept rgy in scratch memory)
  [[maybe_unused]] wvec rgs[NGY];
  int in_off[NIN], in_lds[NIN], in_flag[NIN], gy_off[NGY], gy_lds[NGY];
  // x2 != null: x is the virtual cat([x, x2]) (common.h).  A thread's units all carry the same channel quad
  // (TPB % (CI_T/4) == 0; padding units keep it too), so its source tensor, pixel stride and channel offset are fixed.
  const CatSrc xsrc = DUAL ? cat_src(x, x2, Cin, ca, ci0 + 4 * (tid % (CI_T / 4))) : CatSrc{x, Cin, 0};
#pragma unroll
  for (int i = 0; i < NIN; ++i) {
    const int u = tid + i * TPB;
    const bool real = u < UIN;
    const int uu = real ? u : tid % (CI_T / 4);              // padding unit: pixel 0, this thread's channel quad
    const int q = uu % (CI_T / 4), pix = uu / (CI_T / 4);
    const int iy = pix / IW, ix = pix % IW;
    in_off[i] = (iy * W + ix) * xsrc.stride + 4 * q;
    in_lds[i] = real ? pix * SI + 4 * q : (IH * IW * SI + WTH * TW * SO);          // dummy slot behind both tiles
    in_flag[i] = (iy < PAD ? 1 : 0) | (iy >= WTH + PAD ? 2 : 0) | (ix < PAD ? 4 : 0) | (ix >= TW + PAD ? 8 : 0);
  }
#pragma unroll
  for (int i = 0; i < NGY; ++i) {
    const int u = tid + i * TPB;
    const int q = u % (CO_T / 4), pix = u / (CO_T / 4);
    gy_off[i] = ((pix / TW) * W + (pix % TW)) * Cout + 4 * q;
    gy_lds[i] = pix * SO + 4 * q;
  }
  // first interior pixel of the tile (always inside the image), THIS thread's channel quad: with a virtual-cat source the
  // base pointer carries -coff, which only the quad offset brings back inside the tensor (without it the second part was
  // read 64 B before its first element for the tile at the image origin -- out of bounds when the tensor starts a segment)
  const int safe_off = (PAD * W + PAD) * xsrc.stride + 4 * (tid % (CI_T / 4));
  int pn = t_begin / tiles_img, pty, ptx;                  // cursor of the tile being prefetched
  { const int t = t_begin - pn * tiles_img; pty = t / tiles_x; ptx = t - pty * tiles_x; }
  bool zero[NIN];
  [[maybe_unused]] float4 a_m, a_r, a_g, a_b;                      // INAFF (see conv_mfma_wgrad)
  [[maybe_unused]] const int aq = ci0 + 4 * (tid % (CI_T / 4));
  if (INAFF) { a_g = *(const float4*)(aff.gamma + aq); a_b = *(const float4*)(aff.beta + aq); }
  auto prefetch = [&]() {
    const int flags = (pty == 0 ? 1 : 0) | (pty == tiles_y - 1 ? 2 : 0) | (ptx == 0 ? 4 : 0) | (ptx == tiles_x - 1 ? 8 : 0);
    const float* xb = xsrc.p + (((pn * H + pty * WTH - PAD) * W) + ptx * TW - PAD) * xsrc.stride + ci0 - xsrc.coff;
    const float* gb = gy + (((pn * H + pty * WTH) * W) + ptx * TW) * Cout + co0;
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      zero[i] = (in_flag[i] & flags) != 0;
      rin[i] = *(const wvec*)(xb + (zero[i] ? safe_off : in_off[i]));
    }
#pragma unroll
    for (int i = 0; i < NGY; ++i) rgy[i] = *(const wvec*)(gb + gy_off[i]);
    if constexpr (SC) {
      const float* sb = gs + (((pn * H + pty * WTH) * W) + ptx * TW) * Cout + co0;
#pragma unroll
      for (int i = 0; i < NGY; ++i) rgs[i] = *(const wvec*)(sb + gy_off[i]);
    }
    if (INAFF) {
      a_m = *(const float4*)(aff.mean + (size_t)pn * Cin + aq);
      a_r = *(const float4*)(aff.rstd + (size_t)pn * Cin + aq);
    }
    if (++ptx == tiles_x) { ptx = 0; if (++pty == tiles_y) { pty = 0; ++pn; } }
  };

  [[maybe_unused]] const int stamp_wg = (blockIdx.y == 0 && blockIdx.z == 0) ? (int)blockIdx.x : -1;
  STAMP(0);
  if (t_begin < t_end) prefetch();
  STAMP(1);
  for (int t = t_begin; t < t_end; ++t) {
    __syncthreads();
    if (t - t_begin < 2) { STAMP(2 + 4 * (t - t_begin)); }
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      wvec v = rin[i];
      if (INAFF) {
        v[0] = aff1(v[0], a_m.x, a_r.x, a_g.x, a_b.x, aff.slope); v[1] = aff1(v[1], a_m.y, a_r.y, a_g.y, a_b.y, aff.slope);
        v[2] = aff1(v[2], a_m.z, a_r.z, a_g.z, a_b.z, aff.slope); v[3] = aff1(v[3], a_m.w, a_r.w, a_g.w, a_b.w, aff.slope);
      }
      if (zero[i]) v = WZERO;
      *(wvec*)(in_s + in_lds[i]) = v;
    }
#pragma unroll
    for (int i = 0; i < NGY; ++i) {
      *(wvec*)(gy_s + gy_lds[i]) = rgy[i];
      if constexpr (SC) *(wvec*)(gy_s + gy_lds[i] + 32) = rgs[i];
    }
    __syncthreads();
    if (t - t_begin < 2) { STAMP(3 + 4 * (t - t_begin)); }
    if (t + 1 < t_end) prefetch();
    if (t - t_begin < 2) { STAMP(4 + 4 * (t - t_begin)); }
    {
      const float* ax = in_s + (4 * kq) * SI + (wave >> 1) * 16 + lm;
      const float* bx = gy_s + (4 * kq) * SO + jt * 16 + lm;
      float xr[3][6];
#pragma unroll
      for (int dy = 0; dy < 2; ++dy)
#pragma unroll
        for (int e = 0; e < 6; ++e) xr[dy][e] = ax[(dy * IW + e) * SI];
#pragma unroll
      for (int r = 0; r < WTH; ++r) {
#pragma unroll
        for (int e = 0; e < 6; ++e) xr[(r + 2) % 3][e] = ax[((r + 2) * IW + e) * SI];
        float b[4];
        [[maybe_unused]] float bs[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          b[ks] = bx[(r * TW + ks) * SO];
          if constexpr (SC) bs[ks] = bx[(r * TW + ks) * SO + 32];
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
          for (int k = 0; k < NSLOT; ++k) acc[k] = mfma16(xr[(r + k / KS) % 3][ks + k % KS], b[ks], acc[k]);
          if constexpr (SC) acc_sc = mfma16(xr[(r + 1) % 3][ks + 1], bs[ks], acc_sc);
        }
      }
    }
    if (t - t_begin < 2) { STAMP(5 + 4 * (t - t_begin)); }
  }
  STAMP(10);
  float* out = part + (size_t)split * (SC ? KK + 1 : KK) * Cin * Cout + (size_t)(ci0 + 4 * kq) * Cout + co0 + jt * 16 + lm;
#pragma unroll
  for (int k = 0; k < NSLOT; ++k) {
    const int ti = (wave + 4 * k) >> 1;
    const int tap = ti >> 1, i = ti & 1;
    float* o = out + (tap * Cin + i * 16) * Cout;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      o[r * Cout] = acc[k][r];
    }
  }
  if constexpr (SC) {                           // slab row KK: the shortcut's [Cin][Cout] gradient, this wave's (ci tile, co tile)
    float* o = out + (KK * Cin + (wave >> 1) * 16) * Cout;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r * Cout] = acc_sc[r];
  }
  STAMP(11);
}

// ---- fp16-operand weight gradient (config 5) ------------------------------------------------------------------------------
// gW[tap][ci][co] = sum_p x[p + off(tap)][ci] * gy[p][co] with the PIXELS as the MFMA K dimension: v_mfma_f32_16x16x16_f16
// wants, per lane, four consecutive k (= pixels) of one channel -- the transpose of the pixel-major tiles the staging
// produces.  gfx950's ds_read_b64_tr_b16 does that transpose in the LDS read: per 16-lane group it fetches a block of
// 4 rows (pixels) x 16 columns (channels) and hands lane i column i.  So both operands are staged as fp16 planes
// [16-channel tile][pixel][16] (32-B pixel stride: the 8 pixels a 32-lane half touches fall on 8 x 8 distinct banks) and
// read transposed; one MFMA covers a whole 16-pixel tile row of one tap.  x is staged with its halo, so a tap is a pixel
// offset in the read address.  gy is multiplied by gsc[0] (power of two, smsut_absmax_scale) before the conversion and the
// slab by gsc[1] at the store.
//   TS  (2 x 2 tiles of 16 channels): the 36 accumulator tiles are dealt to the 4 waves, each wave walks all 8 tile rows;
//   !TS (1 x 1, 1 x 2, 2 x 1): every wave keeps all 9*CIT*COT tiles for 2 of the 8 rows, fixed-order combine at the end.
// Full tiles only (H % 8 == 0, W % 16 == 0), Cin % (16*CIT) == 0, Cout % (16*COT) == 0 -- checked by the host.
// SC (r04, config 5): the weight gradient of the block's 1x1 shortcut in the same pass (network/blocks.py:66-80; the fp32 twin is
// conv_mfma_wgrad_ts<.., SC>): a TENTH tap row -- x at the centre-tap offset against the shortcut's gradient gs, staged beside gy
// with the same scale gsc (smsut_absmax_scale2) -- so the slab is [10][Cin][Cout], row 9 = the 1x1 weights' gradient.
// XH (r04): x is an fp16 tensor (the activated a1 of a BasicBlock in half storage) -- copied into the staging planes as it is.
// INAFF (with XH): x is the RAW fp16 conv1 output; lrelu(IN(.)) is applied while staging (as conv_mfma_fwd_p<.., INAFF, .., I16>).
template <int CIT, int COT, bool DUAL, bool SC = false, bool XH = false, bool INAFF = false>
__global__ void __launch_bounds__(TPB)
conv_f16_wgrad(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ part, int N, int H, int W,
               int Cin, int Cout, int tiles_x, int tiles_y, int tiles_per_split, const float* __restrict__ x2, int ca,
               const float* __restrict__ gsc, const float* __restrict__ gsh = nullptr, AffRef aff = AffRef{}) {
  constexpr int KS = 3, KK = 9, PAD = 1;
  constexpr int KR = SC ? 10 : 9;                          // tap rows of the slab
  static_assert(!XH || (!DUAL && !SC), "fp16 x: conv2's weight gradient (plain form)");
  static_assert(!INAFF || (XH && !DUAL && !SC), "input-side IN: the half-storage form, plain input");
  [[maybe_unused]] float4 a_m, a_r, a_g, a_b;              // INAFF: statistics of (image, this thread's channel quad), affine pair
  constexpr bool TS = (CIT == 2 && COT == 2);
  constexpr int IH = WTH + KS - 1, IW = TW + KS - 1;
  constexpr int NPX = IH * IW, NPG = WTH * TW;              // pixels of the haloed x tile / of the gy tile
  constexpr int CI_T = 16 * CIT, CO_T = 16 * COT;
  constexpr int NACC = TS ? KR : KR * CIT * COT;
  extern __shared__ float smem[];
  _Float16* x_h = reinterpret_cast<_Float16*>(smem);       // [CIT][NPX][16]
  _Float16* g_h = x_h + CIT * NPX * 16;                    // [COT][NPG][16]
  [[maybe_unused]] _Float16* s_h = g_h + COT * NPG * 16;   // SC: [COT][NPG][16], the shortcut's gradient
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, kq = lane >> 4;
  const int split = blockIdx.x;
  const int ci0 = blockIdx.y * CI_T, co0 = blockIdx.z * CO_T;
  const int tiles_img = tiles_x * tiles_y;
  const int total_tiles = N * tiles_img;
  const int t_begin = split * tiles_per_split;
  const int t_end = min(t_begin + tiles_per_split, total_tiles);
  const float gs = gsc ? gsc[0] : 1.f, gi = gsc ? gsc[1] : 1.f;

  f32x4 acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto split_store = [&](_Float16* dst, f32x4 v) __attribute__((always_inline)) {
    *(h4*)dst = (h4){(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
  };

  // transposed-read lane address inside a 16-channel plane: group kq takes pixels 4kq .. 4kq+3 of the row segment, lane
  // 4q+p of the group supplies pixel 4kq+q, channels 4p .. 4p+3 (8 bytes)
  const int tr_off = (4 * kq + ((lane >> 2) & 3)) * 16 + 4 * (lane & 3);

  constexpr int UIN = NPX * (CI_T / 4), NIN = (UIN + TPB - 1) / TPB;
  constexpr int UGY = NPG * (CO_T / 4), NGY = UGY / TPB;
  static_assert(UGY % TPB == 0, "gy tile units divide evenly");
  f32x4 rin[XH ? 1 : NIN], rgy[NGY];
  [[maybe_unused]] h4 rinh[XH ? NIN : 1];
  [[maybe_unused]] f32x4 rgs[SC ? NGY : 1];
  int in_off[NIN], in_lds[NIN], in_flag[NIN], gy_off[NGY], gy_lds[NGY];
  const CatSrc xsrc = DUAL ? cat_src(x, x2, Cin, ca, ci0 + 4 * (tid % (CI_T / 4))) : CatSrc{x, Cin, 0};
#pragma unroll
  for (int i = 0; i < NIN; ++i) {
    const int u = tid + i * TPB;
    const bool real = u < UIN;
    const int uu = real ? u : tid % (CI_T / 4);
    const int q = uu % (CI_T / 4), pix = uu / (CI_T / 4);
    const int iy = pix / IW, ix = pix % IW;
    in_off[i] = (iy * W + ix) * xsrc.stride + 4 * q;
    in_lds[i] = real ? ((q >> 2) * NPX + pix) * 16 + 4 * (q & 3) : (CIT * NPX + (SC ? 2 : 1) * COT * NPG) * 16;   // dummy slot behind the images
    in_flag[i] = (iy < PAD ? 1 : 0) | (iy >= WTH + PAD ? 2 : 0) | (ix < PAD ? 4 : 0) | (ix >= TW + PAD ? 8 : 0);
  }
#pragma unroll
  for (int i = 0; i < NGY; ++i) {
    const int u = tid + i * TPB;
    const int q = u % (CO_T / 4), pix = u / (CO_T / 4);
    gy_off[i] = ((pix / TW) * W + (pix % TW)) * Cout + 4 * q;
    gy_lds[i] = ((q >> 2) * NPG + pix) * 16 + 4 * (q & 3);
  }
  const int safe_off = (PAD * W + PAD) * xsrc.stride + 4 * (tid % (CI_T / 4));     // (see conv_mfma_wgrad_ts)
  int pn = t_begin / tiles_img, pty, ptx;
  { const int t = t_begin - pn * tiles_img; pty = t / tiles_x; ptx = t - pty * tiles_x; }
  bool zero[NIN];
  auto prefetch = [&]() {
    const int flags = (pty == 0 ? 1 : 0) | (pty == tiles_y - 1 ? 2 : 0) | (ptx == 0 ? 4 : 0) | (ptx == tiles_x - 1 ? 8 : 0);
    const float* xb = xsrc.p + (((pn * H + pty * WTH - PAD) * W) + ptx * TW - PAD) * xsrc.stride + ci0 - xsrc.coff;
    const float* gb = gy + (((pn * H + pty * WTH) * W) + ptx * TW) * Cout + co0;
    if constexpr (XH) {
      const _Float16* xh = reinterpret_cast<const _Float16*>(xsrc.p) + (xb - xsrc.p);
#pragma unroll
      for (int i = 0; i < NIN; ++i) {
        zero[i] = (in_flag[i] & flags) != 0;
        rinh[i] = *(const h4*)(xh + (zero[i] ? safe_off : in_off[i]));
      }
    } else {
#pragma unroll
      for (int i = 0; i < NIN; ++i) {
        zero[i] = (in_flag[i] & flags) != 0;
        rin[i] = *(const f32x4*)(xb + (zero[i] ? safe_off : in_off[i]));
      }
    }
    if constexpr (INAFF) {                             // every unit of a thread carries the channel quad tid % (CI_T / 4)
      const int ch = ci0 + 4 * (tid % (CI_T / 4));
      a_m = *(const float4*)(aff.mean + (size_t)pn * Cin + ch);
      a_r = *(const float4*)(aff.rstd + (size_t)pn * Cin + ch);
      a_g = *(const float4*)(aff.gamma + ch);
      a_b = *(const float4*)(aff.beta + ch);
    }
#pragma unroll
    for (int i = 0; i < NGY; ++i) rgy[i] = *(const f32x4*)(gb + gy_off[i]);
    if constexpr (SC) {
      const float* sb = gsh + (gb - gy);
#pragma unroll
      for (int i = 0; i < NGY; ++i) rgs[i] = *(const f32x4*)(sb + gy_off[i]);
    }
    if (++ptx == tiles_x) { ptx = 0; if (++pty == tiles_y) { pty = 0; ++pn; } }
  };
  auto tr_read = [&](const _Float16* plane_pix) -> h4 {       // plane_pix: first pixel of the 16-pixel row segment
    typedef s16x4 __attribute__((address_space(3))) lds_s16x4;
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(plane_pix + tr_off));
    return __builtin_bit_cast(h4, v);
  };
  // RS tile rows per MFMA issue: 2 on v_mfma_f32_16x16x32_f16 (comment at mfma32h, conv_mfma.h: k-slots 0..15 = the 16-pixel segment of row r,
  // 16..31 = that of row r + 1 -- the same transposed reads, concatenated; x and gy agree on the order), 1 on the 16-deep instruction
  constexpr int RS = SMSUT_F16_X32 ? 2 : 1;
  static_assert(WTH % 8 == 0, "whole row pairs per wave");
  auto tr_rows = [&](const _Float16* plane_pix, int row_halves) {            // row_halves: halves between the two rows' segments
    if constexpr (RS == 2) {
      const h4 lo = tr_read(plane_pix), up = tr_read(plane_pix + row_halves);
      return (h8)__builtin_shufflevector(lo, up, 0, 1, 2, 3, 4, 5, 6, 7);
    } else {
      (void)row_halves;
      return tr_read(plane_pix);
    }
  };

  if (t_begin < t_end) prefetch();
  for (int t = t_begin; t < t_end; ++t) {
    __syncthreads();
    if constexpr (XH) {
#pragma unroll
      for (int i = 0; i < NIN; ++i) {
        h4 hv = rinh[i];
        if constexpr (INAFF) {
          float4 v = make_float4((float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]);
          v.x = aff1(v.x, a_m.x, a_r.x, a_g.x, a_b.x, aff.slope); v.y = aff1(v.y, a_m.y, a_r.y, a_g.y, a_b.y, aff.slope);
          v.z = aff1(v.z, a_m.z, a_r.z, a_g.z, a_b.z, aff.slope); v.w = aff1(v.w, a_m.w, a_r.w, a_g.w, a_b.w, aff.slope);
          hv = to_h4(v);
        }
        *(h4*)(x_h + in_lds[i]) = zero[i] ? (h4){(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f} : hv;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NIN; ++i) {
        f32x4 v = rin[i];
        split_store(x_h + in_lds[i], zero[i] ? (f32x4){0.f, 0.f, 0.f, 0.f} : v);
      }
    }
#pragma unroll
    for (int i = 0; i < NGY; ++i) split_store(g_h + gy_lds[i], rgy[i] * gs);
    if constexpr (SC) {
#pragma unroll
      for (int i = 0; i < NGY; ++i) split_store(s_h + gy_lds[i], rgs[i] * gs);
    }
    __syncthreads();
    if (t + 1 < t_end) prefetch();
    if constexpr (TS) {
      const int jt = wave & 1;
#pragma unroll
      for (int r = 0; r < WTH; r += RS) {
        const auto b = tr_rows(g_h + (jt * NPG + r * TW) * 16, TW * 16);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const int ti = (wave + 4 * k) >> 1;                  // tap * CIT + i   (wave-uniform)
          const int tap = ti >> 1, i = ti & 1;
          const auto a = tr_rows(x_h + (i * NPX + (r + tap / KS) * IW + tap % KS) * 16, IW * 16);
          acc[k] = mfmak(a, b, acc[k]);
        }
        if constexpr (SC) {                                    // k = 9 is tap row 9 on every wave: (wave + 36) >> 1 = 18 | 19
          const auto bs = tr_rows(s_h + (jt * NPG + r * TW) * 16, TW * 16);
          const auto a = tr_rows(x_h + ((wave >> 1) * NPX + (r + 1) * IW + 1) * 16, IW * 16);
          acc[9] = mfmak(a, bs, acc[9]);
        }
      }
    } else {
#pragma unroll
      for (int rr = 0; rr < WTH / 4; rr += RS) {
        const int r = wave * (WTH / 4) + rr;
        decltype(tr_rows(g_h, 0)) b[COT];
#pragma unroll
        for (int j = 0; j < COT; ++j) b[j] = tr_rows(g_h + (j * NPG + r * TW) * 16, TW * 16);
#pragma unroll
        for (int tap = 0; tap < KK; ++tap)
#pragma unroll
          for (int i = 0; i < CIT; ++i) {
            const auto a = tr_rows(x_h + (i * NPX + (r + tap / KS) * IW + tap % KS) * 16, IW * 16);
#pragma unroll
            for (int j = 0; j < COT; ++j) acc[(tap * CIT + i) * COT + j] = mfmak(a, b[j], acc[(tap * CIT + i) * COT + j]);
          }
        if constexpr (SC) {
          decltype(tr_rows(s_h, 0)) bs[COT];
#pragma unroll
          for (int j = 0; j < COT; ++j) bs[j] = tr_rows(s_h + (j * NPG + r * TW) * 16, TW * 16);
#pragma unroll
          for (int i = 0; i < CIT; ++i) {
            const auto a = tr_rows(x_h + (i * NPX + (r + 1) * IW + 1) * 16, IW * 16);
#pragma unroll
            for (int j = 0; j < COT; ++j) acc[(9 * CIT + i) * COT + j] = mfmak(a, bs[j], acc[(9 * CIT + i) * COT + j]);
          }
        }
      }
    }
  }
  // ---- store: acc[.][r] is (ci = tile*16 + 4*kq + r, co = tile*16 + lm)
  if constexpr (TS) {
    const int jt = wave & 1;
    float* out = part + (size_t)split * KR * Cin * Cout + (size_t)(ci0 + 4 * kq) * Cout + co0 + jt * 16 + lm;
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int ti = (wave + 4 * k) >> 1;
      float* o = out + ((ti >> 1) * Cin + (ti & 1) * 16) * Cout;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r * Cout] = acc[k][r] * gi;
    }
  } else {
    float* red = smem;      // NACC * 64 * 4 floats; combine the 4 waves in a fixed order (wave 0 += 1, 2, 3)
    for (int src = 1; src < 4; ++src) {
      __syncthreads();
      if (wave == src) {
#pragma unroll
        for (int k = 0; k < NACC; ++k) *(f32x4*)(red + ((size_t)k * 64 + lane) * 4) = acc[k];
      }
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int k = 0; k < NACC; ++k) acc[k] += *(const f32x4*)(red + ((size_t)k * 64 + lane) * 4);
      }
    }
    if (wave == 0) {
      float* out = part + (size_t)split * KR * Cin * Cout;
#pragma unroll
      for (int tap = 0; tap < KR; ++tap)
#pragma unroll
        for (int i = 0; i < CIT; ++i)
#pragma unroll
          for (int j = 0; j < COT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              out[((size_t)tap * Cin + ci0 + i * 16 + 4 * kq + r) * Cout + co0 + j * 16 + lm] = acc[(tap * CIT + i) * COT + j][r] * gi;
    }
  }
}

// out[e] = sum_c part[c][e].  COLS float4 columns x (256/COLS) split-lanes per block: each thread strides over the
// splits with 4 independent accumulators (loads in flight), then a fixed-order LDS tree over the lanes (deterministic).
// wsize % 4 == 0 (checked at launch): every access is one aligned float4.  (A scalar tail path that indexed the float4
// accumulator dynamically made the compiler move it to LDS -- 12 KB per block and a 4x slower kernel.)
template <int COLS>
__global__ void __launch_bounds__(TPB)
sum_splits(const float* __restrict__ part, float* __restrict__ out, int wsize, int splits) {
  constexpr int LANES = TPB / COLS;
  __shared__ float4 sm[TPB];
  const int col = threadIdx.x % COLS, sl = threadIdx.x / COLS;
  const int e = (blockIdx.x * COLS + col) * 4;
  float4 t0 = make_float4(0.f, 0.f, 0.f, 0.f), t1 = t0, t2 = t0, t3 = t0;
  if (e < wsize) {
    const float* p = part + e;
    int c = sl;
    for (; c + 3 * LANES < splits; c += 4 * LANES) {
      const float4 v0 = *(const float4*)(p + (size_t)c * wsize);
      const float4 v1 = *(const float4*)(p + (size_t)(c + LANES) * wsize);
      const float4 v2 = *(const float4*)(p + (size_t)(c + 2 * LANES) * wsize);
      const float4 v3 = *(const float4*)(p + (size_t)(c + 3 * LANES) * wsize);
      t0.x += v0.x; t0.y += v0.y; t0.z += v0.z; t0.w += v0.w;
      t1.x += v1.x; t1.y += v1.y; t1.z += v1.z; t1.w += v1.w;
      t2.x += v2.x; t2.y += v2.y; t2.z += v2.z; t2.w += v2.w;
      t3.x += v3.x; t3.y += v3.y; t3.z += v3.z; t3.w += v3.w;
    }
    for (; c < splits; c += LANES) {
      const float4 v = *(const float4*)(p + (size_t)c * wsize);
      t0.x += v.x; t0.y += v.y; t0.z += v.z; t0.w += v.w;
    }
  }
  sm[threadIdx.x] = make_float4((t0.x + t1.x) + (t2.x + t3.x), (t0.y + t1.y) + (t2.y + t3.y),
                                (t0.z + t1.z) + (t2.z + t3.z), (t0.w + t1.w) + (t2.w + t3.w));
  __syncthreads();
  if (sl == 0 && e < wsize) {
    float4 t = sm[col];
    for (int l = 1; l < LANES; ++l) {
      const float4 v = sm[l * COLS + col];
      t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    *(float4*)(out + e) = t;
  }
}

inline void launch_sum_splits(const float* part, float* out, int wsize, int splits, hipStream_t st) {
  // COLS float4 columns (COLS*16 contiguous bytes per split row) x 256/COLS split-lanes per block, ~100-150 blocks:
  // in-process A/B on the layer shapes (scratch/wgrad_ab2.py) -- 4 columns x 64 lanes (the earlier choice for >= 128
  // splits) made the whole weight-gradient call 10-24 % slower at 256^2 / 128^2; 32 / 64 columns win from 32x32 / 64x64
  // weights on (longer contiguous rows per request).
  if (wsize >= 32768) sum_splits<64><<<(wsize + 255) / 256, TPB, 0, st>>>(part, out, wsize, splits);
  else if (wsize >= 8192) sum_splits<32><<<(wsize + 127) / 128, TPB, 0, st>>>(part, out, wsize, splits);
  else sum_splits<16><<<(wsize + 63) / 64, TPB, 0, st>>>(part, out, wsize, splits);
}

// ---- weight gradient on tiny planes (the discriminator's 8x8 / 4x4 levels, 256 -> 256: ugan.py:205-215) -----------------------
// The tiled kernels give every image its own 8x16-pixel tile: on a 4x4 plane 7/8 of each staged tile and of every MFMA is
// padding, and the result still goes through the split-slab sum (56 us for 0.3 GFLOP).  Here the whole batch is the GEMM K
// dimension: gw[tap][ci][co] = sum over ALL N*H*W pixels of x[pixel + tap][ci] * gy[pixel][co]; a wave owns one 16x16 tile
// of one tap split over its pixels, reads its operands straight from global memory (they are L2-resident: <= 2 MB) with
// PW_UNR pixel groups in flight, and the workgroup writes the final value -- no workspace, no second kernel.  W % 4 == 0 (the pixel cursor advances by 4).
constexpr int PW_UNR = 8;
__global__ void __launch_bounds__(TPB)
plane_wgrad(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ gw, int N, int H, int W, int Cin,
            int Cout, const float* __restrict__ x2 = nullptr, int ca = 0) {
  // one workgroup = one 32x32 (ci, co) slab of one tap; every wave computes all four 16x16 tiles of it (two x and two gy
  // loads feed four MFMAs: the kernel is bound by L2 operand traffic, not by latency) on its interleaved share of the
  // pixels; the four waves are combined through LDS in a fixed order
  __shared__ float red[3 * 4 * 64 * 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lm = lane & 15, kq = lane >> 4;
  const int ci0 = blockIdx.x * 32, co0 = blockIdx.y * 32;
  const int tap = blockIdx.z, dy = tap / 3 - 1, dx = tap % 3 - 1;
  const int HW = H * W, P = N * HW;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // x2 != null: x is the virtual cat([x, x2]); each 16-channel tile picks its tensor (uniform per workgroup)
  const CatSrc s0 = cat_src(x, x2, Cin, ca, ci0), s1 = cat_src(x, x2, Cin, ca, ci0 + 16);
  const float* xa0 = s0.p + ci0 + lm - s0.coff;
  const float* xa1 = s1.p + ci0 + 16 + lm - s1.coff;
  const float* gb = gy + co0 + lm;
  constexpr int BLK = 4 * PW_UNR;                            // pixels per wave per round
  for (int p0 = wave * BLK; p0 < P; p0 += 4 * BLK) {
    // pixel cursor of this lane: (n, y, x) of pixel p0 + kq, advanced by 4 pixels per group without divisions
    // (W % 4 == 0: the column wraps at most once per step); three divisions per round, none per group
    const int pk = p0 + kq;
    int cn = pk / HW;
    const int r = pk - cn * HW;
    int cy = r / W, cx = r - cy * W;
    float a[PW_UNR][2], b[PW_UNR][2];
#pragma unroll
    for (int u = 0; u < PW_UNR; ++u) {
      const int p = p0 + 4 * u + kq;                         // this lane's pixel (the MFMA k index) of group u
      const int yy = cy + dy, xx = cx + dx;
      const bool ok = p < P;
      const bool in = ok && yy >= 0 && yy < H && xx >= 0 && xx < W;
      const size_t pix = (size_t)((cn * H + yy) * W + xx);
      const float* gp = gb + (size_t)p * Cout;
      a[u][0] = in ? xa0[pix * s0.stride] : 0.f; a[u][1] = in ? xa1[pix * s1.stride] : 0.f;
      b[u][0] = ok ? gp[0] : 0.f; b[u][1] = ok ? gp[16] : 0.f;
      cx += 4;
      if (cx >= W) { cx -= W; if (++cy == H) { cy = 0; ++cn; } }
    }
#pragma unroll
    for (int u = 0; u < PW_UNR; ++u)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(a[u][i], b[u][j], acc[i][j]);
  }
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) *(f32x4*)(red + (((wave - 1) * 4 + t) * 64 + lane) * 4) = acc[t >> 1][t & 1];
  }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4 v = acc[t >> 1][t & 1];
#pragma unroll
      for (int w4 = 0; w4 < 3; ++w4) v += *(const f32x4*)(red + ((w4 * 4 + t) * 64 + lane) * 4);
      float* o = gw + ((size_t)tap * Cin + ci0 + (t >> 1) * 16 + 4 * kq) * Cout + co0 + (t & 1) * 16 + lm;
#pragma unroll
      for (int r = 0; r < 4; ++r) o[(size_t)r * Cout] = v[r];
    }
  }
}

// weight gradient of the 4x4 s1 p1 conv: gW[tap][ci][co] = sum over output pixels of x[p + tap - 1][ci] * gy[p][co].  A workgroup
// owns a 16 x 16*COT slab for all 16 taps and walks 8x16-OUTPUT-pixel tiles of a split; waves split the tile rows, fixed-order
// combine, per-split slabs summed by sum_splits (as conv_mfma_wgrad).
template <int COT>
__global__ void __launch_bounds__(TPB)
conv_k4_wgrad(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ part, int N, int Hi, int Wi,
              int Ho, int Wo, int Cin, int Cout, int tiles_x, int tiles_y, int tiles_per_split) {
  constexpr int KS = 4, KK = 16, PAD = 1;
  constexpr int IH = WTH + KS - 1, IW = TW + KS - 1;
  constexpr int CO_T = 16 * COT, SI = 16, SO = (CO_T % 32 == 16) ? CO_T : CO_T + 16;
  constexpr int NACC = KK * COT;
  extern __shared__ float smem[];
  float* in_s = smem;                         // [IH][IW][SI]
  float* gy_s = smem + IH * IW * SI;          // [WTH][TW][SO]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, kq = lane >> 4;
  const int split = blockIdx.x, ci0 = blockIdx.y * 16, co0 = blockIdx.z * CO_T;
  const int tiles_img = tiles_x * tiles_y, total_tiles = N * tiles_img;
  const int t_begin = split * tiles_per_split, t_end = min(t_begin + tiles_per_split, total_tiles);
  f32x4 acc[NACC];
#pragma unroll
  for (int k = 0; k < NACC; ++k) acc[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
  constexpr int NIN = (IH * IW * 4 + TPB - 1) / TPB, NGY = (WTH * TW * (CO_T / 4) + TPB - 1) / TPB;
  float4 rin[NIN], rgy[NGY];
  auto prefetch = [&](int t) {
    const int n_img = t / tiles_img, rem = t % tiles_img;
    const int y0 = (rem / tiles_x) * WTH, x0 = (rem % tiles_x) * TW;
    const float* xin = x + (size_t)n_img * Hi * Wi * Cin;
    const float* gin = gy + (size_t)n_img * Ho * Wo * Cout;
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      const int u = tid + i * TPB, q = u & 3, pix = u >> 2;
      const int gy_ = y0 + pix / IW - PAD, gx_ = x0 + pix % IW - PAD, c = ci0 + 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (u < IH * IW * 4 && c < Cin && gy_ >= 0 && gy_ < Hi && gx_ >= 0 && gx_ < Wi)
        v = *(const float4*)(xin + ((size_t)gy_ * Wi + gx_) * Cin + c);
      rin[i] = v;
    }
#pragma unroll
    for (int i = 0; i < NGY; ++i) {
      const int u = tid + i * TPB, q = u % (CO_T / 4), pix = u / (CO_T / 4);
      const int gy_ = y0 + pix / TW, gx_ = x0 + pix % TW, c = co0 + 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (u < WTH * TW * (CO_T / 4) && c < Cout && gy_ < Ho && gx_ < Wo) v = *(const float4*)(gin + ((size_t)gy_ * Wo + gx_) * Cout + c);
      rgy[i] = v;
    }
  };
  if (t_begin < t_end) prefetch(t_begin);
  for (int t = t_begin; t < t_end; ++t) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      const int u = tid + i * TPB;
      if (u < IH * IW * 4) *(float4*)(in_s + (u >> 2) * SI + 4 * (u & 3)) = rin[i];
    }
#pragma unroll
    for (int i = 0; i < NGY; ++i) {
      const int u = tid + i * TPB;
      if (u < WTH * TW * (CO_T / 4)) *(float4*)(gy_s + (u / (CO_T / 4)) * SO + 4 * (u % (CO_T / 4))) = rgy[i];
    }
    __syncthreads();
    if (t + 1 < t_end) prefetch(t + 1);
#pragma unroll
    for (int rr = 0; rr < WTH / 4; ++rr) {
      const int r = wave * (WTH / 4) + rr;
#pragma unroll
      for (int ks = 0; ks < TW / 4; ++ks) {
        const int px = ks * 4 + kq;
        float b[COT];
#pragma unroll
        for (int j = 0; j < COT; ++j) b[j] = gy_s[(r * TW + px) * SO + j * 16 + lm];
#pragma unroll
        for (int tap = 0; tap < KK; ++tap) {
          const float a = in_s[((r + tap / KS) * IW + px + tap % KS) * SI + lm];
#pragma unroll
          for (int j = 0; j < COT; ++j) acc[tap * COT + j] = mfma16(a, b[j], acc[tap * COT + j]);
        }
      }
    }
  }
  float* red = smem;
  for (int src = 1; src < 4; ++src) {
    __syncthreads();
    if (wave == src) {
#pragma unroll
      for (int k = 0; k < NACC; ++k) *(f32x4*)(red + ((size_t)k * 64 + lane) * 4) = acc[k];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int k = 0; k < NACC; ++k) acc[k] += *(const f32x4*)(red + ((size_t)k * 64 + lane) * 4);
    }
  }
  if (wave == 0) {
    float* out = part + (size_t)split * KK * Cin * Cout;
#pragma unroll
    for (int tap = 0; tap < KK; ++tap)
#pragma unroll
      for (int j = 0; j < COT; ++j) {
        const int co = co0 + j * 16 + lm;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ci = ci0 + 4 * kq + r;
          if (ci < Cin && co < Cout) out[((size_t)tap * Cin + ci) * Cout + co] = acc[tap * COT + j][r];
        }
      }
  }
}

// ---- weight gradient: plan, kernel ladder (families in the order wgrad_select tries them) and launchers -----------------------------
enum WgradFamily {
  WF_NONE,     // no kernel for this shape and form
  WF_RR,       // register-row kernel (conv_wgrad_rr.hip): no LDS staging, no barrier in the main loop
  WF_PLANE,    // plane_wgrad: whole-batch GEMM of a tiny plane, final values written directly (no slabs)
  WF_C8,       // row-split kernel, 8-channel form (tap pairs share an accumulator tile) ...
  WF_C8_SC,    // ... with the fused shortcut
  WF_TS,       // tap-split kernel (32 x 32 channel slabs, full tiles)
  WF_ROWS,     // row-split kernel conv_mfma_wgrad<KS, cit, cot>
};
struct WgradPlan {
  int cit, cot, splits, tiles_per_split, tiles_x, tiles_y;     // splits: slabs the launch writes
  WgradFamily fam = WF_NONE;
  int rows = 0;           // tap rows of a slab: KS*KS, + 1 with the fused shortcut
  int ws_splits = 0;      // slabs a workspace must hold: the MAXIMUM of the register-row rung's and of the rung below it (below_rr)
};

constexpr int WGRAD_TARGET11 = 768;     // workgroups the split plan aims for: 16 x 16 slabs ...
constexpr int WGRAD_TARGET = 512;       // ... and the wider ones
constexpr int WGRAD_CAP_MFLOATS = 8;    // bound on the split slabs sum_splits re-reads (M floats)

WgradPlan plan_wgrad(int N, int H, int W, int Cin, int Cout) {
  WgradPlan p;
  // (2x2 slabs need 178 VGPRs + 144 AGPRs = one wave per SIMD, yet measured faster than 2x1 / 1x2 slabs at two waves
  //  per SIMD, and forcing __launch_bounds__(256, 2) spills -- r01 sweeps, profiles/r01_notes.md)
  p.cit = (Cin > 16) ? 2 : 1;
  p.cot = (Cout > 16) ? 2 : 1;
  p.tiles_x = (W + TW - 1) / TW;
  p.tiles_y = (H + WTH - 1) / WTH;
  const int total = N * p.tiles_x * p.tiles_y;
  const int slabs = ((Cin + 16 * p.cit - 1) / (16 * p.cit)) * ((Cout + 16 * p.cot - 1) / (16 * p.cot));
  // PMC (r01, 64->64 @64^2): with 1024 two-tile workgroups the kernel averaged < 1 resident wave per SIMD -- the
  // per-workgroup fixed cost (descriptor setup, first-tile latency, cross-wave combine, slab store) dominated.  The
  // 144..186-VGPR variants fit 2 workgroups per CU, so ONE resident round of 512 workgroups with more tiles each.
  const int target = (p.cit == 1 && p.cot == 1) ? WGRAD_TARGET11 : WGRAD_TARGET;
  int want = (target + slabs - 1) / slabs;
  // ... but keep the per-split slabs that sum_splits has to re-read bounded (default 32 MB = 8M floats; an 8 MB cap
  // left the 64->64 layers with 208 workgroups for 256 CUs: PMC showed < 1 resident wave per SIMD).
  const int64_t wsz = (int64_t)Cin * Cout * 9;
  int cap = (int)(((int64_t)WGRAD_CAP_MFLOATS << 20) / wsz);
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  if (want > total) want = total;
  if (want < 1) want = 1;
  p.tiles_per_split = (total + want - 1) / want;
  p.splits = (total + p.tiles_per_split - 1) / p.tiles_per_split;
  return p;
}

#ifndef PLANE_WGRAD_MAX_HW
#define PLANE_WGRAD_MAX_HW 64      // 8x8 planes too: 57 -> 35 us at B16 256->256 vs the tap-split kernel (scratch/plane_wgrad_ab.py)
#endif
// planes small enough for the whole-batch GEMM form
inline bool plane_wgrad_applies(int N, int H, int W, int Cin, int Cout) {
  return H * W <= PLANE_WGRAD_MAX_HW && W % 4 == 0 && Cin % 32 == 0 && Cout % 32 == 0 && (int64_t)N * H * W <= 4096 &&
         (int64_t)N * H * W * (Cin > Cout ? Cin : Cout) < (1ll << 31);
}
inline bool wgrad_channels_ok(int Cin, int Cout) { return Cin >= 4 && (Cin % 4) == 0 && Cout >= 4 && (Cout % 4) == 0; }

// THE kernel ladder of the fp32 weight gradient: the launch (wgrad_run) and every `_supported` / `_ws` query read this one plan, so
// no launch writes more slabs than its caller was told to allocate.  below_rr: the ladder under the register-row rung, where a call
// continues when that launcher declines.  WF_NONE / WF_PLANE plans keep the row-split tile split: the `_ws` queries answer for them too.
WgradPlan wgrad_select(const WgradKey& k, int KS, bool below_rr = false) {
  if (k.N <= 0 || k.H <= 0 || k.W <= 0) return WgradPlan{};
  WgradPlan p = plan_wgrad(k.N, k.H, k.W, k.Cin, k.Cout);
  p.rows = KS * KS + (k.sc ? 1 : 0);
  p.ws_splits = p.splits;
  if ((KS != 1 && KS != 3) || !wgrad_channels_ok(k.Cin, k.Cout)) return p;
  if ((k.aff && (k.cat || k.sc)) || (KS == 1 && (k.aff || k.sc))) return p;      // forms no kernel has
  if (KS == 1) { p.fam = WF_ROWS; return p; }
  const int rr = smsut_wgrad_rr_splits(k);               // the register-row kernel plans its own split count
  if (rr > p.ws_splits) p.ws_splits = rr;
  if (rr && !below_rr) { p.fam = WF_RR; p.splits = rr; return p; }
  if (plane_wgrad_applies(k.N, k.H, k.W, k.Cin, k.Cout) && !k.aff) {
    if (!k.sc) p.fam = WF_PLANE;
    return p;
  }
  if (k.Cin == 8 && !k.cat && !k.aff) {                  // (fused shortcut: up to two 16-channel result tiles)
    p.fam = !k.sc ? WF_C8 : k.Cout <= 32 ? WF_C8_SC : WF_NONE;
    return p;
  }
  // whole 32 x 32 channel slabs, full tiles: the fused shortcut wins 6-14 us per call there; on the 16-channel slabs it pushed the
  // row-split kernel over 256 VGPRs and ran 0-7 us SLOWER (scratch/wsc_ab.py): two kernels, unless the register-row kernel takes them
  if (k.H % WTH == 0 && k.W % TW == 0 && k.Cin % 32 == 0 && k.Cout % 32 == 0 &&
      (int64_t)k.N * k.H * k.W * (k.Cin > k.Cout ? k.Cin : k.Cout) < (1ll << 31))
    p.fam = WF_TS;
  else if (!k.sc) p.fam = WF_ROWS;
  return p;
}
inline int64_t wgrad_ws_floats(const WgradKey& k, int KS) {
  const WgradPlan p = wgrad_select(k, KS);
  return (int64_t)p.ws_splits * p.rows * k.Cin * k.Cout;
}

// row-split kernel; the form follows the call and the plan's family.  -1: no instantiation (nothing launched).  up = 2
// (ConvTranspose2x2 only): gy is the 2x larger tensor, up * up tap groups in blockIdx.y
template <int KS, int CIT, int COT>
int launch_wgrad(const WgradCall& c, const WgradPlan& p, int up) {
  constexpr int IH = WTH + KS - 1, IW = TW + KS - 1;
  constexpr int CI_T = 16 * CIT, CO_T = 16 * COT;
  constexpr int SI = (CI_T % 32 == 16) ? CI_T : CI_T + 16;
  constexpr int SO = (CO_T % 32 == 16) ? CO_T : CO_T + 16;
  constexpr size_t stage = (size_t)(IH * IW * SI + WTH * TW * SO) * sizeof(float);
  constexpr size_t red = (size_t)KS * KS * CIT * COT * 64 * 4 * sizeof(float);
  constexpr size_t sh = stage > red ? stage : red;
  static_assert(sh <= 64 * 1024, "LDS budget");
  const int nci = (c.Cin + CI_T - 1) / CI_T;
  const dim3 grid(p.splits, nci * up * up, (c.Cout + CO_T - 1) / CO_T);
  auto go = [&](auto kern, size_t lds) {
    kern<<<grid, TPB, lds, c.stream>>>((const float*)c.x, c.gy, c.part, c.N, c.H, c.W, c.Cin, c.Cout, p.tiles_x, p.tiles_y,
                                       p.tiles_per_split, up, nci, c.x2, c.ca, c.aff ? *c.aff : AffRef{}, c.gs);
    return 0;
  };
  const bool c8 = p.fam == WF_C8 || p.fam == WF_C8_SC;
  if (c.gs && p.fam != WF_C8_SC) return -1;
  if (c8) {
    if constexpr (KS == 3 && CIT == 1) {
      constexpr size_t stage_sc = (size_t)(IH * IW * SI + 2 * WTH * TW * SO) * sizeof(float);
      constexpr size_t red_sc = (size_t)((KS * KS + 1) / 2 + 1) * CIT * COT * 64 * 4 * sizeof(float);
      constexpr size_t sh_sc = stage_sc > red_sc ? stage_sc : red_sc;
      static_assert(sh_sc <= 64 * 1024, "LDS budget");
      if (c.aff || c.x2 || up != 1 || c.Cin != 8) return -1;
      return c.gs ? go(conv_mfma_wgrad<KS, CIT, COT, false, false, true, true>, sh_sc)
                  : go(conv_mfma_wgrad<KS, CIT, COT, false, false, true>, sh);
    } else return -1;
  }
  if (c.aff) return (c.x2 || up != 1) ? -1 : go(conv_mfma_wgrad<KS, CIT, COT, false, true>, sh);
  return c.x2 ? go(conv_mfma_wgrad<KS, CIT, COT, true>, sh) : go(conv_mfma_wgrad<KS, CIT, COT, false>, sh);
}
int launch_wgrad_rows(const WgradCall& c, const WgradPlan& p, int up = 1) {
  if (c.KS == 1)
    return p.cit == 1 ? (p.cot == 1 ? launch_wgrad<1, 1, 1>(c, p, up) : launch_wgrad<1, 1, 2>(c, p, up))
                      : (p.cot == 1 ? launch_wgrad<1, 2, 1>(c, p, up) : launch_wgrad<1, 2, 2>(c, p, up));
  return p.cit == 1 ? (p.cot == 1 ? launch_wgrad<3, 1, 1>(c, p, up) : launch_wgrad<3, 1, 2>(c, p, up))
                    : (p.cot == 1 ? launch_wgrad<3, 2, 1>(c, p, up) : launch_wgrad<3, 2, 2>(c, p, up));
}

// tap-split kernel: {cat, aff, sc} of the call -> conv_mfma_wgrad_ts<DUAL, INAFF, SC>
int launch_wgrad_ts(const WgradCall& c, const WgradPlan& p) {
  constexpr size_t sh = (size_t)((WTH + 2) * (TW + 2) * WTS_STRIDE + WTH * TW * WTS_STRIDE + 4) * sizeof(float);
  constexpr size_t sh_sc = (size_t)((WTH + 2) * (TW + 2) * WTS_STRIDE + WTH * TW * WTS_STRIDE_SC + 4) * sizeof(float);
  const dim3 grid(p.splits, c.Cin / 32, c.Cout / 32);
  auto go = [&](auto kern, size_t lds) {
    kern<<<grid, TPB, lds, c.stream>>>((const float*)c.x, c.gy, c.part, c.N, c.H, c.W, c.Cin, c.Cout, p.tiles_x, p.tiles_y,
                                       p.tiles_per_split, c.x2, c.ca, c.aff ? *c.aff : AffRef{}, c.gs);
    return 0;
  };
  if (c.gs) {
    if (c.aff) return -1;
    [[maybe_unused]] static const bool attr = [] {       // (once: the shortcut forms' LDS tile is over the 64 KB default)
      (void)hipFuncSetAttribute((const void*)conv_mfma_wgrad_ts<false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh_sc);
      (void)hipFuncSetAttribute((const void*)conv_mfma_wgrad_ts<true, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh_sc);
      return true;
    }();
    return c.x2 ? go(conv_mfma_wgrad_ts<true, false, true>, sh_sc) : go(conv_mfma_wgrad_ts<false, false, true>, sh_sc);
  }
  if (c.aff) return c.x2 ? -1 : go(conv_mfma_wgrad_ts<false, true>, sh);
  return c.x2 ? go(conv_mfma_wgrad_ts<true>, sh) : go(conv_mfma_wgrad_ts<false>, sh);
}

// what every weight-gradient entry point shares: the operands (x2 nullable: ca then counts for nothing), shape and stream of a call ...
inline WgradCall wgrad_call(const void* x, const float* x2, int ca, const float* gy, float* part, int N, int H, int W, int Cin, int Cout,
                            void* stream) {
  WgradCall c;
  c.x = x; c.x2 = x2; c.ca = x2 ? ca : 0; c.gy = gy; c.part = part;
  c.N = N; c.H = H; c.W = W; c.Cin = Cin; c.Cout = Cout; c.stream = (hipStream_t)stream;
  return c;
}
// ... and its end: rc of a launcher (-1 = form not covered, nothing launched), then the plan's slabs summed into gw in a fixed order
inline int wgrad_reduce(int rc, const WgradCall& c, const WgradPlan& p, float* gw) {
  SMSUT_REQUIRE(rc == 0);
  launch_sum_splits(c.part, gw, p.rows * c.Cin * c.Cout, p.splits, c.stream);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

// One fp32 weight-gradient call down the ladder.  gw null (measurement entry points): stop before the reduction and return the slab
// count.  Paired and measurement calls are the register-row kernel's alone.
int wgrad_run(const WgradCall& c, float* gw) {
  SMSUT_REQUIRE(c.x && c.gy && c.part && c.N > 0 && c.H > 0 && c.W > 0);
  SMSUT_REQUIRE(!c.x2 || (c.ca > 0 && c.ca < c.Cin && c.ca % 16 == 0 && (c.Cin - c.ca) % 4 == 0));
  const WgradKey k = c.key();
  WgradPlan p = wgrad_select(k, c.KS);
  if (p.fam == WF_RR && smsut_wgrad_rr_launch(c) != 0) p = wgrad_select(k, c.KS, /*below_rr=*/true);   // declined: on down the ladder
  if (c.b || !gw) SMSUT_REQUIRE(p.fam == WF_RR);
  if (!gw) return hipGetLastError() == hipSuccess ? p.splits : SMSUT_EINVAL;
  switch (p.fam) {
    case WF_NONE: return SMSUT_EINVAL;
    case WF_RR: return wgrad_reduce(0, c, p, gw);
    case WF_TS: return wgrad_reduce(launch_wgrad_ts(c, p), c, p, gw);
    case WF_PLANE:                                       // final values written directly: no split-slab sum
      plane_wgrad<<<dim3(c.Cin / 32, c.Cout / 32, 9), TPB, 0, c.stream>>>((const float*)c.x, c.gy, gw, c.N, c.H, c.W, c.Cin, c.Cout,
                                                                        c.x2, c.ca);
      SMSUT_LAUNCH_CHECK();
      return SMSUT_OK;
    default: return wgrad_reduce(launch_wgrad_rows(c, p), c, p, gw);
  }
}

// ---- fp16-operand 3x3 weight gradient (conv_f16_wgrad): full 8x16-pixel tiles and whole 16-channel tiles only -----------------------
inline bool wgrad_f16_shape_ok(int N, int H, int W, int Cin, int Cout) {
  return N > 0 && H > 0 && W > 0 && H % WTH == 0 && W % TW == 0 && Cin % 16 == 0 && Cout % 16 == 0 &&
         (int64_t)N * H * W * (Cin > Cout ? Cin : Cout) < (1ll << 31);
}
WgradPlan plan_wgrad_f16(int N, int H, int W, int Cin, int Cout, bool sc) {
  WgradPlan p = plan_wgrad(N, H, W, Cin, Cout);
  p.cit = (Cin % 32 == 0) ? 2 : 1;
  p.cot = (Cout % 32 == 0) ? 2 : 1;
  p.rows = sc ? 10 : 9;
  return p;
}
// forms: plain / virtual cat, each with the fused shortcut (10 tap rows); fp16 x (x_f16), plain or with the input-side IN
template <int CI, int CO>
int launch_wgrad_f16(const WgradCall& c, const WgradPlan& p) {
  constexpr int NPX = (WTH + 2) * (TW + 2), NPG = WTH * TW;
  const bool sc = c.gs != nullptr;
  const size_t stage = (size_t)((CI * NPX + (sc ? 2 : 1) * CO * NPG) * 16 + 8) * sizeof(_Float16);
  const size_t red = (CI == 2 && CO == 2) ? 0 : (size_t)p.rows * CI * CO * 64 * 4 * sizeof(float);
  const dim3 grid(p.splits, c.Cin / (16 * CI), c.Cout / (16 * CO));
  auto go = [&](auto kern) {
    kern<<<grid, TPB, stage > red ? stage : red, c.stream>>>((const float*)c.x, c.gy, c.part, c.N, c.H, c.W, c.Cin, c.Cout, p.tiles_x,
                                                             p.tiles_y, p.tiles_per_split, c.x2, c.ca, c.gsc, c.gs,
                                                             c.aff ? *c.aff : AffRef{});
    return 0;
  };
  if (c.x_f16) {
    if (c.x2 || sc) return -1;
    return c.aff ? go(conv_f16_wgrad<CI, CO, false, false, true, true>) : go(conv_f16_wgrad<CI, CO, false, false, true>);
  }
  if (c.aff) return -1;
  if (sc) return c.x2 ? go(conv_f16_wgrad<CI, CO, true, true>) : go(conv_f16_wgrad<CI, CO, false, true>);
  return c.x2 ? go(conv_f16_wgrad<CI, CO, true, false>) : go(conv_f16_wgrad<CI, CO, false, false>);
}
int wgrad_f16_run(const WgradCall& c, float* gw) {
  SMSUT_REQUIRE(c.x && c.gy && gw && c.part && wgrad_f16_shape_ok(c.N, c.H, c.W, c.Cin, c.Cout));
  SMSUT_REQUIRE(!c.x2 || (c.ca > 0 && c.ca < c.Cin && c.ca % 16 == 0));
  const WgradPlan p = plan_wgrad_f16(c.N, c.H, c.W, c.Cin, c.Cout, c.gs != nullptr);
  const int rc = p.cit == 2 ? (p.cot == 2 ? launch_wgrad_f16<2, 2>(c, p) : launch_wgrad_f16<2, 1>(c, p))
                            : (p.cot == 2 ? launch_wgrad_f16<1, 2>(c, p) : launch_wgrad_f16<1, 1>(c, p));
  return wgrad_reduce(rc, c, p, gw);
}

}  // namespace

extern "C" {

#ifdef SMSUT_STAMPS    // this file's own stamp buffer (conv_mfma.h); conv_mfma.hip's is set by smsut_dbg_set_stamps
int smsut_dbg_wgrad_stamps(void* buf, int base) {
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_base), &base, sizeof(base));
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &buf, sizeof(buf));
}
#endif
#ifdef SMSUT_DBG_SUM   // scratch/ diagnostic builds only: the split-slab reduction as its own call
int smsut_dbg_sum_splits(const float* part, float* out, int wsize, int splits, void* stream) {
  launch_sum_splits(part, out, wsize, splits, (hipStream_t)stream);
  return 0;
}
#endif

int smsut_conv2d_wgrad_mfma_supported(int KS, int stride, int pad, int Cin, int Cout) {
  return (KS == 1 || KS == 3) && stride == 1 && pad == (KS - 1) / 2 && wgrad_channels_ok(Cin, Cout);
}

// workspace floats: splits * KS*KS*Cin*Cout.  Serves the plain, virtual-cat and input-side-IN forms, which plan the same splits.
int64_t smsut_conv2d_wgrad_mfma_ws(int N, int H, int W, int Cin, int Cout, int KS) {
  return wgrad_ws_floats(WgradKey{N, H, W, Cin, Cout, false, false, false}, KS);
}

// gw [KS*KS][Cin][Cout] = sum over pixels of x (x) gy
int smsut_conv2d_wgrad_mfma(const float* x, const float* gy, float* gw, float* workspace, int N, int H, int W, int Cin,
                            int Cout, int KS, void* stream) {
  SMSUT_REQUIRE(gw);
  WgradCall c = wgrad_call(x, nullptr, 0, gy, workspace, N, H, W, Cin, Cout, stream);
  c.KS = KS;
  return wgrad_run(c, gw);
}

// 3x3 weight gradient whose x operand is lrelu(IN(x)) of the tensor passed (see smsut_conv2d_fwd_mfma_stats_inaff);
// workspace as smsut_conv2d_wgrad_mfma_ws(N, H, W, Cin, Cout, 3).
int smsut_conv2d_wgrad_mfma_inaff(const float* x, const float* gy, float* gw, float* workspace, const float* mean,
                                  const float* rstd, const float* gamma, const float* beta, float slope, int N, int H, int W,
                                  int Cin, int Cout, void* stream) {
  SMSUT_REQUIRE(gw && mean && rstd && gamma && beta);
  const AffRef a{mean, rstd, gamma, beta, slope};
  WgradCall c = wgrad_call(x, nullptr, 0, gy, workspace, N, H, W, Cin, Cout, stream);
  c.aff = &a;
  return wgrad_run(c, gw);
}

// Measurement entry point (bench.py's roofline leg): the FIRST of the two launches of smsut_conv2d_wgrad_mfma_inaff alone -- the
// register-row kernel writing its per-split slabs into the workspace, without the sum_splits reduction -- so that HIP events
// bracket exactly the kernel rocprofv3 lists.  Returns the number of slabs written (> 0), or a negative value when the shape is
// not one the register-row kernel takes.  mean == NULL: plain form (x is the operand itself).
int smsut_conv2d_wgrad_mfma_slabs(const float* x, const float* gy, float* workspace, const float* mean, const float* rstd,
                                  const float* gamma, const float* beta, float slope, int N, int H, int W, int Cin, int Cout,
                                  void* stream) {
  SMSUT_REQUIRE(!mean || (rstd && gamma && beta));
  const AffRef a{mean, rstd, gamma, beta, slope};
  WgradCall c = wgrad_call(x, nullptr, 0, gy, workspace, N, H, W, Cin, Cout, stream);
  c.aff = mean ? &a : nullptr;
  return wgrad_run(c, nullptr);
}

// conv1's 3x3 weight gradient AND the 1x1 shortcut's (network/blocks.py:66-80: both convs read x) in one pass:
//   gw10 [10][Cin][Cout]: rows 0..8 = sum_p x[p + tap] (x) gy[p]  (as smsut_conv2d_wgrad_mfma), row 9 = sum_p x[p] (x) gs[p].
// xb nullable: non-null = x is the virtual cat([xa, xb]), ca channels in xa.  workspace: smsut_conv2d_wgrad_sc_ws floats.
int smsut_conv2d_wgrad_sc_supported(int N, int H, int W, int Cin, int Cout) {
  return wgrad_select(WgradKey{N, H, W, Cin, Cout, false, false, true}, 3).fam != WF_NONE;
}
int64_t smsut_conv2d_wgrad_sc_ws(int N, int H, int W, int Cin, int Cout) {
  return wgrad_ws_floats(WgradKey{N, H, W, Cin, Cout, false, false, true}, 3);
}
int smsut_conv2d_wgrad_mfma_sc(const float* xa, const float* xb, int ca, const float* gy, const float* gs, float* gw10,
                               float* workspace, int N, int H, int W, int Cin, int Cout, void* stream) {
  SMSUT_REQUIRE(gw10 && gs);
  WgradCall c = wgrad_call(xa, xb, ca, gy, workspace, N, H, W, Cin, Cout, stream);
  c.gs = gs;
  return wgrad_run(c, gw10);
}

// Weight gradient with x = the virtual cat([xa, xb]) (xa [N,H,W,ca], xb [N,H,W,Cin-ca], ca % 16 == 0) read in place;
// workspace as smsut_conv2d_wgrad_mfma_ws(N, H, W, Cin, Cout, KS).
int smsut_conv2d_wgrad_mfma_cat(const float* xa, const float* xb, int ca, const float* gy, float* gw, float* workspace,
                                int N, int H, int W, int Cin, int Cout, int KS, void* stream) {
  SMSUT_REQUIRE(gw && xb);
  WgradCall c = wgrad_call(xa, xb, ca, gy, workspace, N, H, W, Cin, Cout, stream);
  c.KS = KS;
  return wgrad_run(c, gw);
}

// PAIRED 3x3 weight gradient (r05): gw = wgrad(set A) + wgrad(set B) in ONE launch of the register-row kernel, for two image sets
// that went through the SAME conv -- the two generator passes of a uganConsis iteration (G(x_real), G(x_fake); reference
// uganConsisTrainer.py:152,159) differentiate every layer twice with 16 slices each; paired, a layer's weight gradient is one launch
// over 32 slices (the fixed part of a launch -- prologue, first-row latency, combine, slab store, the split-slab sum -- is paid once
// and the split plan is the 32-slice one).  Form flags as the single-set entry points: x2 (virtual cat, ca channels in x), mean /
// rstd (x is the RAW conv output, lrelu(IN(.)) applied in flight: gamma, beta, slope shared -- same layer), gs (fused 1x1 shortcut,
// gw holds 10 rows); each present in BOTH sets or in neither.
int smsut_conv2d_wgrad_pair_supported(int NA, int NB, int H, int W, int Cin, int Cout, int cat, int aff, int sc) {
  return NA > 0 && NB > 0 && wgrad_select(WgradKey{NA + NB, H, W, Cin, Cout, cat != 0, aff != 0, sc != 0}, 3).fam == WF_RR;
}
int64_t smsut_conv2d_wgrad_pair_ws(int NA, int NB, int H, int W, int Cin, int Cout, int cat, int aff, int sc) {
  return (int64_t)smsut_wgrad_rr_splits(WgradKey{NA + NB, H, W, Cin, Cout, cat != 0, aff != 0, sc != 0}) * (sc ? 10 : 9) * Cin * Cout;
}
// what the paired entry point and its measurement twin share: one call over NA + NB images (the launcher checks set B against set A)
static int wgrad_pair_run(const WgradSetB& sa, const WgradSetB& sb, int ca, const float* gamma, const float* beta, float slope, float* gw,
                          float* workspace, int H, int W, int Cin, int Cout, void* stream) {
  const bool aff = sa.mean != nullptr;
  SMSUT_REQUIRE(aff == (sa.rstd != nullptr) && (!aff || (gamma && beta)));
  const AffRef a{sa.mean, sa.rstd, gamma, beta, slope};
  WgradCall c = wgrad_call(sa.x, sa.x2, ca, sa.gy, workspace, sa.n + sb.n, H, W, Cin, Cout, stream);
  c.gs = sa.gs;
  c.aff = aff ? &a : nullptr;
  c.b = &sb;
  return wgrad_run(c, gw);
}
int smsut_conv2d_wgrad_pair(const float* xA, const float* x2A, const float* gyA, const float* gsA, const float* meanA,
                            const float* rstdA, int NA, const float* xB, const float* x2B, const float* gyB, const float* gsB,
                            const float* meanB, const float* rstdB, int NB, int ca, const float* gamma, const float* beta, float slope,
                            float* gw, float* workspace, int H, int W, int Cin, int Cout, void* stream) {
  SMSUT_REQUIRE(gw);
  return wgrad_pair_run(WgradSetB{xA, x2A, gyA, gsA, meanA, rstdA, NA}, WgradSetB{xB, x2B, gyB, gsB, meanB, rstdB, NB}, ca, gamma, beta,
                        slope, gw, workspace, H, W, Cin, Cout, stream);
}

// Measurement entry point (bench.py's roofline leg), the paired twin of smsut_conv2d_wgrad_mfma_slabs: the register-row kernel of
// smsut_conv2d_wgrad_pair ALONE (input-side-IN or plain form, no virtual cat / shortcut), slabs left in the workspace, no reduction.
// Returns the number of slabs written (> 0) or a negative value.
int smsut_conv2d_wgrad_pair_slabs(const float* xA, const float* gyA, const float* meanA, const float* rstdA, int NA, const float* xB,
                                  const float* gyB, const float* meanB, const float* rstdB, int NB, const float* gamma,
                                  const float* beta, float slope, float* workspace, int H, int W, int Cin, int Cout, void* stream) {
  return wgrad_pair_run(WgradSetB{xA, nullptr, gyA, nullptr, meanA, rstdA, NA}, WgradSetB{xB, nullptr, gyB, nullptr, meanB, rstdB, NB}, 0,
                        gamma, beta, slope, nullptr, workspace, H, W, Cin, Cout, stream);
}

// 3x3 weight gradient with fp16 operands (conv_f16_wgrad): full 8x16-pixel tiles and whole 16-channel tiles only
int smsut_conv2d_wgrad_f16_supported(int N, int H, int W, int Cin, int Cout) { return wgrad_f16_shape_ok(N, H, W, Cin, Cout); }
int64_t smsut_conv2d_wgrad_f16_ws(int N, int H, int W, int Cin, int Cout) {
  return (int64_t)plan_wgrad_f16(N, H, W, Cin, Cout, false).splits * 9 * Cin * Cout;
}
// x2 (nullable): x is the virtual cat([x, x2]) with ca channels in x (ca % 16 == 0)
int smsut_conv2d_wgrad_f16(const float* x, const float* x2, int ca, const float* gy, float* gw, float* workspace,
                           const float* gsc, int N, int H, int W, int Cin, int Cout, void* stream) {
  WgradCall c = wgrad_call(x, x2, ca, gy, workspace, N, H, W, Cin, Cout, stream);
  c.gsc = gsc;
  return wgrad_f16_run(c, gw);
}
// ... with x stored as fp16 [N,H,W,Cin] (half storage: conv2's weight gradient of a BasicBlock reads the activated a1): same bits
int smsut_conv2d_wgrad_f16_xh(const void* x16, const float* gy, float* gw, float* workspace, const float* gsc, int N, int H, int W,
                              int Cin, int Cout, void* stream) {
  WgradCall c = wgrad_call(x16, nullptr, 0, gy, workspace, N, H, W, Cin, Cout, stream);
  c.gsc = gsc; c.x_f16 = true;
  return wgrad_f16_run(c, gw);
}
// ... with x the RAW fp16 conv1 output, lrelu(IN(.)) applied while staging (half-storage twin of smsut_conv2d_wgrad_mfma_inaff)
int smsut_conv2d_wgrad_f16_xh_inaff(const void* y1_16, const float* gy, float* gw, float* workspace, const float* gsc,
                                    const float* mean, const float* rstd, const float* gamma, const float* beta, float slope, int N,
                                    int H, int W, int Cin, int Cout, void* stream) {
  SMSUT_REQUIRE(mean && rstd && gamma && beta);
  const AffRef a{mean, rstd, gamma, beta, slope};
  WgradCall c = wgrad_call(y1_16, nullptr, 0, gy, workspace, N, H, W, Cin, Cout, stream);
  c.gsc = gsc; c.x_f16 = true; c.aff = &a;
  return wgrad_f16_run(c, gw);
}
// ... and the block's 1x1 shortcut weight gradient in the same pass: gw10 [10][Cin][Cout], rows 0..8 = the 3x3 taps, row 9 = the
// shortcut's (as smsut_conv2d_wgrad_mfma_sc); gsc = smsut_absmax_scale2(gy, gs).
int smsut_conv2d_wgrad_sc_f16_supported(int N, int H, int W, int Cin, int Cout) { return wgrad_f16_shape_ok(N, H, W, Cin, Cout); }
int64_t smsut_conv2d_wgrad_sc_f16_ws(int N, int H, int W, int Cin, int Cout) {
  return (int64_t)plan_wgrad_f16(N, H, W, Cin, Cout, true).splits * 10 * Cin * Cout;
}
int smsut_conv2d_wgrad_sc_f16(const float* x, const float* x2, int ca, const float* gy, const float* gs, float* gw10,
                              float* workspace, const float* gsc, int N, int H, int W, int Cin, int Cout, void* stream) {
  SMSUT_REQUIRE(gs && gsc);
  WgradCall c = wgrad_call(x, x2, ca, gy, workspace, N, H, W, Cin, Cout, stream);
  c.gs = gs; c.gsc = gsc;
  return wgrad_f16_run(c, gw10);
}

// ---- 4x4 stride-1 pad-1 convolution (forward / data-gradient: smsut_conv2d_k4_fwd, conv_mfma.hip) ----------------------------
// (H, W) are always the extents of the conv's FORWARD INPUT; its output is (H-1) x (W-1).
static WgradPlan plan_wgrad_k4(int N, int H, int W, int Cin, int Cout) {
  WgradPlan p;
  p.cit = 1; p.cot = (Cout > 16) ? 2 : 1;
  p.tiles_x = (W - 1 + TW - 1) / TW;
  p.tiles_y = (H - 1 + WTH - 1) / WTH;
  const int total = N * p.tiles_x * p.tiles_y;
  const int slabs = ((Cin + 15) / 16) * ((Cout + 16 * p.cot - 1) / (16 * p.cot));
  int want = (512 + slabs - 1) / slabs;
  const int64_t wsz = (int64_t)Cin * Cout * 16;
  int cap = (int)(((int64_t)8 << 20) / wsz);
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  if (want > total) want = total;
  if (want < 1) want = 1;
  p.tiles_per_split = (total + want - 1) / want;
  p.splits = (total + p.tiles_per_split - 1) / p.tiles_per_split;
  return p;
}
int64_t smsut_conv2d_k4_wgrad_ws(int N, int H, int W, int Cin, int Cout) {
  return (int64_t)plan_wgrad_k4(N, H, W, Cin, Cout).splits * 16 * Cin * Cout;
}
// x [N,H,W,Cin], gy [N,H-1,W-1,Cout] -> gw [4][4][Cin][Cout]
int smsut_conv2d_k4_wgrad(const float* x, const float* gy, float* gw, float* workspace, int N, int H, int W, int Cin, int Cout,
                          void* stream) {
  SMSUT_REQUIRE(x && gy && gw && workspace && N > 0 && H > 1 && W > 1 && smsut_conv2d_k4_supported(Cin, Cout));
  SMSUT_REQUIRE((int64_t)N * H * W * (Cin > Cout ? Cin : Cout) < (1ll << 31));
  hipStream_t st = (hipStream_t)stream;
  const WgradPlan p = plan_wgrad_k4(N, H, W, Cin, Cout);
  constexpr int IH = WTH + 3, IW = TW + 3;
  if (p.cot == 2) {
    constexpr size_t stage = (size_t)(IH * IW * 16 + WTH * TW * 48) * sizeof(float), red = (size_t)32 * 64 * 4 * sizeof(float);
    conv_k4_wgrad<2><<<dim3(p.splits, (Cin + 15) / 16, (Cout + 31) / 32), TPB, stage > red ? stage : red, st>>>(
        x, gy, workspace, N, H, W, H - 1, W - 1, Cin, Cout, p.tiles_x, p.tiles_y, p.tiles_per_split);
  } else {
    constexpr size_t stage = (size_t)(IH * IW * 16 + WTH * TW * 16) * sizeof(float), red = (size_t)16 * 64 * 4 * sizeof(float);
    conv_k4_wgrad<1><<<dim3(p.splits, (Cin + 15) / 16, (Cout + 15) / 16), TPB, stage > red ? stage : red, st>>>(
        x, gy, workspace, N, H, W, H - 1, W - 1, Cin, Cout, p.tiles_x, p.tiles_y, p.tiles_per_split);
  }
  launch_sum_splits(workspace, gw, 16 * Cin * Cout, p.splits, st);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

int64_t smsut_convT2x2_wgrad_mfma_ws(int N, int H, int W, int Cin, int Cout) {
  const WgradPlan p = plan_wgrad(N, H, W, Cin, Cout);
  return (int64_t)p.splits * 4 * Cin * Cout;
}

int smsut_convT2x2_wgrad_mfma(const float* x, const float* gy, float* gw, float* workspace, int N, int H, int W, int Cin,
                              int Cout, void* stream) {
  SMSUT_REQUIRE(x && gy && gw && workspace && N > 0 && H > 0 && W > 0 && smsut_convT2x2_mfma_supported(Cin, Cout));
  WgradCall c = wgrad_call(x, nullptr, 0, gy, workspace, N, H, W, Cin, Cout, stream);
  c.KS = 1;
  WgradPlan p = plan_wgrad(N, H, W, Cin, Cout);
  p.rows = 4;                                   // four taps, each a 1x1 weight gradient against its quarter of the 2x larger gy
  return wgrad_reduce(launch_wgrad_rows(c, p, /*up=*/2), c, p, gw);
}

}  // extern "C"
