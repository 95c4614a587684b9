// Implicit-GEMM convolution on the gfx950 matrix cores, fp32 in / fp32 accumulate
// (v_mfma_f32_16x16x4_f32: exact f32, bit-identical to an fmaf chain -- MI355X_MICROARCH.md "Matrix cores").
//
// Covers every stride-1 "same" convolution of the hot path with a K-dimension (input channels) that is a
// multiple of 4: the 3x3 and 1x1 convs of BasicBlock / BottleBlock (network/blocks.py:10-16,53-117), i.e.
// > 97 % of the U-Net / ugan / discriminator FLOPs.  NHWC activations, [KH][KW][Cin][Cout] weights.
//
//   forward      out[p, n] = sum_{tap, k} in[p + off(tap), k] * W[tap][k][n]
//   data-grad    the same kernel on gy with W read transposed and tap-flipped (``transposed`` = 1)
//   weight-grad  gW[tap][k][n] = sum_p in[p + off(tap), k] * gy[p, n]   (GEMM with the pixels as K)
//
// This file holds the forward / data-gradient family: conv_mfma_fwd, conv_mfma_fwd_p, the 4x4 and ConvTranspose2x2 forward and
// data-gradient, their launchers, selection and `_supported` / `_tiles` / `_form` queries.  The weight gradient is conv_mfma_wgrad.hip
// (LDS-staged kernels) and conv_wgrad_rr.hip (register-row kernel); the device primitives both families use are conv_mfma.h.
//
// Forward tiling (one 256-thread workgroup = 4 waves, one per SIMD):
//   * output tile TH rows x 16 pixels x CO_T = 16*NTN channels; each wave owns MR rows x NR channel tiles,
//     i.e. MR*NR accumulators of 16x16 (pixels along one image row are the MFMA M dimension);
//   * the input channels are walked in chunks of 16; per chunk the haloed input tile [(TH+KS-1)][16+KS-1][16]
//     and the weights [taps][16][CO_T] are staged in LDS once and reused by all taps / waves;
//   * A fragments are ONE ds_read_b128 per (tap,row): lane (m, kq) reads channels 4kq..4kq+3 of pixel m and
//     feeds them to 4 consecutive MFMAs (the k order inside a 16-chunk is permuted, which a sum does not
//     see); B fragments likewise from a [tap][kq][n][4] image.  Pixel stride 24 floats (= 8 mod 16) and the
//     n-major weight image make both reads bank-conflict-free for the b128 lane groups (MICROARCH "LDS").
#include "conv_mfma.h"
#include "conv_wino.h"
#include <stdlib.h>
#include <type_traits>

namespace {

constexpr int CK = 16;       // input-channel chunk staged per LDS pass
constexpr int SPIX = 24;     // floats between consecutive pixels of the staged input tile (16 + 8 pad)

// (r03: the Winograd transforms written as inline-asm v_pk_add_f32 with neg modifiers halve their VALU count -- the compiler
//  scalarises a vector fsub whose lanes feed MFMA operands one by one -- but the hazard recogniser does not see inside inline
//  asm: the VALU-write -> MFMA-read wait states were missing and the results were wrong.  Plain vector arithmetic it is.)
__device__ __forceinline__ f32x4 sub4(f32x4 a, f32x4 b) { return a - b; }
__device__ __forceinline__ f32x4 add4(f32x4 a, f32x4 b) { return a + b; }

constexpr int SPIXH = 24;    // halves between consecutive pixels of the staged fp16 input tile
constexpr int WROWH = 24;    // halves between consecutive output channels of the staged fp16 weights ([n][16 k] + pad)
__device__ __forceinline__ h4 to_h4s(float4 v, float s) {
  return (h4){(_Float16)(v.x * s), (_Float16)(v.y * s), (_Float16)(v.z * s), (_Float16)(v.w * s)};
}

// CKW (fp16 operands only; r05): channels staged per LDS pass.  32: one pass moves 128 contiguous bytes per pixel and per weight row --
// whole cache lines, where the 16-channel pass takes half of each line (the vector-memory path bounds these kernels: the data-gradient
// form, whose weight rows are read along k, ran at half the forward form's rate on the 128 / 256-channel levels) -- and the 32-deep MFMA
// takes the 32 channels of ONE tap per issue: 9 issues per chunk and tile pair instead of 2 x 5.  Kdim % 32 == 0 (host).
template <int KS, int TH, int WM, int WN, int NTN, bool F16 = false, int MW = TW, int CKW = 16>
__global__ void __launch_bounds__(TPB)
conv_mfma_fwd(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, int H, int W, int Kdim,
              int Ndim, int tiles_x, int transposed, int isc, int osc, int G, int nz, float* __restrict__ stats,
              const float* __restrict__ x2 = nullptr, float* __restrict__ y2 = nullptr, int split = 0,
              const float* __restrict__ gsc = nullptr) {
  // F16: fp16 operands, converted while staging (block comment above mfma16h, conv_mfma.h); gsc (nullable) = {s, 1/s} of a gradient input.
  // MW (16, 8, 4): width of the pixel tile.  One MFMA M-tile is 16 pixels = (16 / MW) rows x MW columns, so on the
  // discriminator's 8x8 / 4x4 planes (network/ugan.py:205-215) every MFMA row is a real pixel: with 16-wide tiles half (8x8) or
  // three quarters (4x4) of each MFMA multiplied padding columns (r01: "dense pixel packing").  Plain conv forms only.
  // x2 (nullable, regular conv only): the input is the virtual cat([x, x2]) of two Kdim/2-channel tensors (common.h); the
  // select is per 16-channel chunk, i.e. uniform.  y2 / split (nullable): result channels >= split go to y2 (see
  // conv_mfma_fwd_p).
  // stats (nullable): per-workgroup InstanceNorm partials [n][tile][Ndim][2] = {sum, sum of squares} of this tile's
  // outputs, in the layout in_moments_final<0> (norm.hip) consumes -- the statistics pass over y is then not needed.
  // (H, W) is the compute grid.  Regular conv: isc = osc = G = 1.  ConvTranspose2x2 forward: osc = 2 and
  // blockIdx.z also enumerates the 4 output taps.  ConvTranspose2x2 data-gradient: isc = 2, G = 4 input taps.
  constexpr int KK = KS * KS;
  constexpr int PAD = (KS - 1) / 2;
  constexpr int IH = TH + KS - 1, IW = MW + KS - 1;
  constexpr int CO_T = 16 * NTN;
  constexpr int RPT = TW / MW;                 // rows of one 16-pixel M-tile
  constexpr int MT = TH / RPT;                 // M-tiles per pixel tile
  constexpr int MR = MT / WM, NR = NTN / WN;
  static_assert(WM * WN == 4 && TH % RPT == 0 && MT % WM == 0 && MR >= 1 && NTN % WN == 0, "wave grid");
  static_assert(MW == 16 || MW == 8 || MW == 4, "M-tile width");
  static_assert(CKW == 16 || (CKW == 32 && F16 && SMSUT_F16_X32), "32-channel passes: fp16 operands on the 32-deep instruction");
  constexpr int Q = CKW / 4;                   // float4 units per pixel / per weight row of one pass
  constexpr int PXH = CKW == 32 ? 40 : SPIXH;  // halves between pixels / weight rows of the fp16 images (80 B: eight lanes' 16-byte
  constexpr int WRH = CKW == 32 ? 40 : WROWH;  // reads 20 banks apart -> 32 distinct banks, as the 48-B stride of the 16-channel image)
  extern __shared__ float smem[];
  float* in_s = smem;                        // [IH][IW][SPIX]
  float* w_s = smem + IH * IW * SPIX;        // [KK][4][CO_T][4]
  [[maybe_unused]] _Float16* in_h = reinterpret_cast<_Float16*>(smem);      // F16: [IH][IW][PXH]
  [[maybe_unused]] _Float16* w_h = reinterpret_cast<_Float16*>(w_s);        // F16: [KK][CO_T][WRH]
  [[maybe_unused]] const float gs = (F16 && gsc) ? gsc[0] : 1.f, gi = (F16 && gsc) ? gsc[1] : 1.f;

  const bool accum = (transposed & 2) != 0;     // y += conv(x) instead of y = conv(x) (second gradient path of a block)
  transposed &= 1;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int lm = lane & 15, kq = lane >> 4;
  const int tile = blockIdx.x;
  const int ty = tile / tiles_x, tx = tile % tiles_x;
  const int n_img = blockIdx.y;
  [[maybe_unused]] const int stamp_wg = blockIdx.z == 0 ? (int)(blockIdx.y * gridDim.x + blockIdx.x) : -1;
  const int tapo = blockIdx.z / nz;            // output tap (transposed conv forward), else 0
  const int co0 = (blockIdx.z % nz) * CO_T;
  const int y0 = ty * TH, x0 = tx * MW;
  // this lane's pixel inside an M-tile (A operand: pixel index = lm) and the pixels of its accumulator elements (4*kq + r)
  const int a_row = lm / MW, a_col = lm % MW;
  const int Wi = W * isc;
  const int KSTR = x2 ? Kdim / 2 : Kdim;       // pixel stride of the input tensor(s)
  const float* xin = x + (size_t)n_img * H * isc * Wi * KSTR;
  const float* xin2 = x2 ? x2 + (size_t)n_img * H * isc * Wi * KSTR : xin;
  w += (size_t)tapo * KK * Kdim * Ndim;

  f32x4 acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Software pipeline over (tap group g, 16-channel chunk c0): the NEXT chunk's global loads are issued into
  // registers right after the current chunk has been published to LDS, so their latency hides under the MFMAs.
  constexpr int NI = (IH * IW * Q + TPB - 1) / TPB;       // float4 units of the input tile per thread
  constexpr int NW = (KK * Q * CO_T + TPB - 1) / TPB;     // float4 units of the weight chunk per thread
  float4 rin[NI], rw[NW];
  const int nchunk = (Kdim + CKW - 1) / CKW;
  const int nsteps = G * nchunk;
  // per-thread unit descriptors, computed once (integer div/mod is ~40 VALU instructions each on CDNA)
  int in_off[NI], in_q[NI];        // element offset of the pixel inside one image (tap group 0), or -1; channel quad
  int w_off[NW], w_k[NW], w_dst[NW];   // element offset inside one tap-group chunk (c0 = 0), or -1; k of the unit; its LDS offset
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int u = tid + i * TPB;
    const int q = u % Q, pix = u / Q;
    const int iy = pix / IW, ix = pix % IW;
    const int gy_ = y0 + iy - PAD, gx_ = x0 + ix - PAD;
    const bool ok = u < IH * IW * Q && gy_ >= 0 && gy_ < H && gx_ >= 0 && gx_ < W;
    in_off[i] = ok ? ((gy_ * isc) * Wi + gx_ * isc) * KSTR + 4 * q : -1;
    in_q[i] = 4 * q;
  }
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int u = tid + i * TPB;
    // unit u = (tap, k quad, n).  Forward: n fastest -- consecutive lanes read consecutive output channels of one k row (Cout-contiguous
    // memory).  Data-gradient (weights read transposed: [ng][k] rows of Kdim floats): the k quad fastest -- four lanes cover the 64
    // contiguous bytes a chunk takes from one row; with n fastest every lane of a wave touched its own cache line (r05: the fp16-operand
    // data-gradients of the 128 / 256-channel levels ran at 130-240 TF against 350-490 TF forward, scratch/cfg_f16_probe.py).
    const int n = transposed ? (u / Q) % CO_T : u % CO_T;
    const int k4 = transposed ? (u % Q) : (u / CO_T) % Q;
    const int tap = u / (Q * CO_T);
    const int ng = co0 + n;
    const bool ok = u < KK * Q * CO_T && ng < Ndim;
    w_k[i] = 4 * k4;
    w_dst[i] = F16 ? (tap * CO_T + n) * WRH + 4 * k4 : ((tap * 4 + k4) * CO_T + n) * 4;
    w_off[i] = !ok ? -1 : (!transposed ? (tap * Kdim + 4 * k4) * Ndim + ng : ((KK - 1 - tap) * Ndim + ng) * Kdim + 4 * k4);
  }

  auto prefetch = [&](int step) {
    const int g = step / nchunk, c0 = (step % nchunk) * CKW;
    const float* wg = w + (size_t)g * KK * Kdim * Ndim + (transposed ? c0 : c0 * Ndim);
    const bool second = x2 && c0 >= KSTR;
    const float* xg = (second ? xin2 : xin) + ((size_t)(g >> 1) * Wi + (g & 1)) * KSTR + (second ? c0 - KSTR : c0);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in_off[i] >= 0 && c0 + in_q[i] < Kdim) v = *(const float4*)(xg + in_off[i]);
      rin[i] = v;
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (w_off[i] >= 0 && c0 + w_k[i] < Kdim) {
        const float* p = wg + w_off[i];
        if (!transposed) { v.x = p[0]; v.y = p[Ndim]; v.z = p[2 * (size_t)Ndim]; v.w = p[3 * (size_t)Ndim]; }
        else v = *(const float4*)p;
      }
      rw[i] = v;
    }
  };

  STAMP(0);
  prefetch(0);
  STAMP(1);
  for (int step = 0; step < nsteps; ++step) {
    __syncthreads();                         // every wave is done reading the previous chunk
    if (step < 2) { STAMP(2 + 4 * step); }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int u = tid + i * TPB;
      if (u < IH * IW * Q) {
        if (F16) *(h4*)(in_h + (u / Q) * PXH + 4 * (u % Q)) = to_h4s(rin[i], gs);
        else *(float4*)(in_s + (u >> 2) * SPIX + 4 * (u & 3)) = rin[i];
      }
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int u = tid + i * TPB;
      if (u < KK * Q * CO_T) {
        // four consecutive k of output channel n of one tap, at the unit's place in [tap][k quad][n][4] (fp16: [tap][n][16 k + pad])
        if (F16) *(h4*)(w_h + w_dst[i]) = to_h4(rw[i]);
        else *(float4*)(w_s + w_dst[i]) = rw[i];
      }
    }
    __syncthreads();
    if (step < 2) { STAMP(3 + 4 * step); }
    if (step + 1 < nsteps) prefetch(step + 1);
    if (step < 2) { STAMP(4 + 4 * step); }
    // ---- MFMA over taps
    if constexpr (CKW == 32) {
      // the 32 channels of one tap per issue: lane (lm, kq) holds channels 8kq .. 8kq+7 of its pixel / its output channel
#pragma unroll
      for (int tap = 0; tap < KK; ++tap) {
        const int kh = tap / KS, kw = tap % KS;
        h8 a[MR], b[NR];
#pragma unroll
        for (int i = 0; i < MR; ++i)
          a[i] = *(const h8*)(in_h + (((wm * MR + i) * RPT + a_row + kh) * IW + a_col + kw) * PXH + 8 * kq);
#pragma unroll
        for (int j = 0; j < NR; ++j)
          b[j] = *(const h8*)(w_h + ((size_t)tap * CO_T + (wn * NR + j) * 16 + lm) * WRH + 8 * kq);
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < NR; ++j) acc[i][j] = mfma32h(a[i], b[j], acc[i][j]);
      }
    } else if constexpr (F16 && SMSUT_F16_X32) {
      // tap pairs on the 32-deep instruction (comment at mfma32h); a lone last tap multiplies zeros in the upper k-slots
      const bool hi = kq >= 2;
      const int ko = 8 * (kq & 1);
      const h8 zero8 = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
#pragma unroll
      for (int p = 0; p < (KK + 1) / 2; ++p) {
        const bool solo = 2 * p + 1 >= KK;
        const int tlo = 2 * p, thi = solo ? 2 * p : 2 * p + 1;
        const int tap = hi ? thi : tlo;
        const int kh = hi ? thi / KS : tlo / KS, kw = hi ? thi % KS : tlo % KS;
        h8 a[MR], b[NR];
#pragma unroll
        for (int i = 0; i < MR; ++i) {
          a[i] = *(const h8*)(in_h + (((wm * MR + i) * RPT + a_row + kh) * IW + a_col + kw) * SPIXH + ko);
          if (solo && hi) a[i] = zero8;
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          b[j] = *(const h8*)(w_h + ((size_t)tap * CO_T + (wn * NR + j) * 16 + lm) * WROWH + ko);
          if (solo && hi) b[j] = zero8;
        }
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < NR; ++j) acc[i][j] = mfma32h(a[i], b[j], acc[i][j]);
      }
    } else if constexpr (F16) {
#pragma unroll
      for (int tap = 0; tap < KK; ++tap) {
        const int kh = tap / KS, kw = tap % KS;
        h4 a[MR], b[NR];
#pragma unroll
        for (int i = 0; i < MR; ++i)
          a[i] = *(const h4*)(in_h + (((wm * MR + i) * RPT + a_row + kh) * IW + a_col + kw) * SPIXH + 4 * kq);
#pragma unroll
        for (int j = 0; j < NR; ++j)
          b[j] = *(const h4*)(w_h + ((size_t)tap * CO_T + (wn * NR + j) * 16 + lm) * WROWH + 4 * kq);
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < NR; ++j) acc[i][j] = mfma16h(a[i], b[j], acc[i][j]);
      }
    } else
#pragma unroll
    for (int tap = 0; tap < KK; ++tap) {
      const int kh = tap / KS, kw = tap % KS;
      f32x4 a[MR], b[NR];
#pragma unroll
      for (int i = 0; i < MR; ++i)
        a[i] = *(const f32x4*)(in_s + (((wm * MR + i) * RPT + a_row + kh) * IW + a_col + kw) * SPIX + 4 * kq);
#pragma unroll
      for (int j = 0; j < NR; ++j)
        b[j] = *(const f32x4*)(w_s + (((tap * 4 + kq) * CO_T) + (wn * NR + j) * 16 + lm) * 4);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < NR; ++j) acc[i][j] = mfma16(a[i][s], b[j][s], acc[i][j]);
    }
    if (step < 2) { STAMP(5 + 4 * step); }
  }
  // ---- epilogue: acc[i][j][r] is pixel (row wm*MR+i, col 4*kq + r), channel (wn*NR+j)*16 + lm
  if (F16) {
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j) acc[i][j] *= gi;
  }
  if (stats) {
    __syncthreads();                          // LDS is free again: reuse it for the cross-wave combine
    float* red = smem;                        // [WM][CO_T][2]
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int i = 0; i < MR; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = 4 * kq + r;                                     // pixel of this accumulator element inside its M-tile
          const bool ok = y0 + (wm * MR + i) * RPT + p / MW < H && x0 + p % MW < W;
          const float v = ok ? acc[i][j][r] : 0.f;
          s1 += v; s2 += v * v;
        }
      }
      s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
      s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
      if (kq == 0) {
        red[(wm * CO_T + (wn * NR + j) * 16 + lm) * 2] = s1;
        red[(wm * CO_T + (wn * NR + j) * 16 + lm) * 2 + 1] = s2;
      }
    }
    __syncthreads();
    if (tid < CO_T && co0 + tid < Ndim) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int m = 0; m < WM; ++m) { s1 += red[(m * CO_T + tid) * 2]; s2 += red[(m * CO_T + tid) * 2 + 1]; }
      float* o = stats + (((size_t)n_img * gridDim.x + tile) * Ndim + co0 + tid) * 2;
      o[0] = s1; o[1] = s2;
    }
  }
  STAMP(10);
  const int Wo = W * osc;
#pragma unroll
  for (int i = 0; i < MR; ++i) {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int co = co0 + (wn * NR + j) * 16 + lm;
      if (co >= Ndim) continue;
      const bool hi = y2 && co0 + (wn * NR + j) * 16 >= split;           // uniform per (workgroup, j)
      const int os = !y2 ? Ndim : (hi ? Ndim - split : split);
      float* yout = (hi ? y2 : y) + (size_t)n_img * H * osc * Wo * os + (hi ? co - split : co);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = 4 * kq + r;
        const int gy_ = y0 + (wm * MR + i) * RPT + p / MW, gx_ = x0 + p % MW;
        if (gy_ < H && gx_ < W) {
          float* o = yout + ((size_t)(gy_ * osc + (tapo >> 1)) * Wo + gx_ * osc + (tapo & 1)) * os;
          *o = accum ? acc[i][j][r] + *o : acc[i][j][r];
        }
      }
    }
  }
  STAMP(11);
}

// ------------------------------------------------------------------------------------- persistent forward / dgrad
// Same tile and fragment layout as conv_mfma_fwd, restructured for the small-Cin / large-image layers (the 256^2 and
// 128^2 levels), where one tile is only 1-4 channel chunks of work.  s_memtime stamps of conv_mfma_fwd<3,8,4,1,1> at
// N16 256^2 32->16 (profiles/r01_notes.md): a workgroup lives ~29.5k cycles of which only 8.2k are its two MFMA phases;
// index set-up (3.4k), issuing the next chunk's loads (3.2k), the two barriers around the LDS publish (4.2k per chunk)
// and the stats + store epilogue (5.4k) are serial phases of an in-order wave, and with 4 waves per SIMD the matrix
// pipe idles 42 % of the time.  Here a workgroup
//   * stages the WHOLE weight block [taps][Kdim][CO_T] in LDS once and computes its staging descriptors once,
//   * walks a contiguous range of (image, tile) items,
//   * and inside ONE straight-line region per chunk issues the next chunk's loads, the PREVIOUS item's statistics and
//     stores (its accumulators are kept in a second register set) and the current chunk's MFMAs, so the scheduler can
//     put the overhead instructions into the shadow of the MFMAs (24 of every 32 issue cycles are free).
// Regular stride-1 "same" 3x3 conv; W % 16 == 0, H % TH == 0, Ndim % (16*NTN) == 0, Kdim == 16*NCH (checked by the host).
// BST ("backward statistics", data-gradient of conv2 inside a BasicBlock): the result g is the gradient w.r.t.
// a1 = LeakyReLU(IN(y1)); the epilogue multiplies it by the activation mask recomputed from y1 (in_affine), stores
// gz = g * mask, and emits the per-tile partials {sum gz, sum gz * xhat} of the InstanceNorm backward -- the separate
// reduction pass over (g, y1) disappears (in_moments_partial<1>: 4.5 % of the uganConsis iteration).
// Input-side InstanceNorm + LeakyReLU ("INAFF"): the conv input is a = lrelu(in_affine(x; mean[n,c], rstd[n,c], gamma[c],
// beta[c])) of the tensor actually read -- conv2 of a BasicBlock and its weight gradient read the raw conv1 output y1 and
// normalise it while staging, so a1 is never written to or read from HBM.  Same in_affine() fma as norm.hip: same bits.
// (AffRef, BstRef and ScRef, the kernel arguments of these forms: common.h; aff1, the per-element form: conv_mfma.h)

// Pixel stride (floats) of the staged input tile of the Winograd form: 20 = 5 x 16 B.  A lane of the transform reads the
// channel quad kq of pixel (2*tc + b, 2*tr + a) of its 4x4 window; 16-byte slots (pixel * 5 + kq) mod 16 over the 16 tiles of
// a wave take 8 distinct values twice (every ds_read_b128 address is a multiple of 16 B and the tile origins are 2 pixels
// apart, so 2-way is the floor for this lane-to-tile map; 24 would be 4-way).
constexpr int SPIXW = 20;

template <int KS, int TH, int NTN, int NCH, bool STATS, bool ACC, bool BST = false, bool DUAL = false, bool INAFF = false,
          bool F16 = false, bool K8 = false, bool SC = false, bool SC2 = false, bool N8 = false, bool WINO = false, bool O16 = false, bool I16 = false,
          bool FIN = false>
__global__ void __launch_bounds__(TPB) __attribute__((amdgpu_waves_per_eu(WINO ? 2 : 1, WINO ? 2 : 8)))
conv_mfma_fwd_p(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, int N, int H, int W,
                int Ndim, int tiles_x, int tiles_img, int items_per_wg, int transposed, float* __restrict__ stats,
                BstRef bst = BstRef{}, float* __restrict__ y2 = nullptr, int split = 0,
                const float* __restrict__ x2 = nullptr, AffRef aff = AffRef{}, const float* __restrict__ gsc = nullptr,
                ScRef sc = ScRef{}, FinRef fin = FinRef{}) {
  // FIN / fin (common.h): the workgroup whose partials complete an image finalises its InstanceNorm statistics in this launch (a
  // template flag, so that the instantiations without it keep their registers: the tail's loads in flight would set the count of
  // the 64-128-register forms)
  static_assert(!FIN || ((STATS || BST) && !F16 && !N8), "in-launch finalize: fp32 statistics / BST forms");
  // SC: conv1 of a BasicBlock AND the block's 1x1 shortcut conv in one pass (network/blocks.py:66-80: both read the block input).
  // The 1x1 conv is the centre tap with its own weights: the A fragments of tap (1,1) feed a second accumulator set (+1/9 MFMAs),
  // the epilogue stores the second result sc.y and its InstanceNorm partials sc.stats -- the separate 1x1 kernel and its re-read
  // of the block input (HBM-bound, 5 FLOP/B) disappear.  Forward statistics forms (plain or virtual-cat input), fp32.
  static_assert(!SC || (STATS && !ACC && !BST && !INAFF && KS == 3), "fused shortcut: forward statistics forms");
  static_assert(!(SC && F16 && (K8 || WINO)), "fused shortcut with fp16 operands: the direct 16-channel-chunk form");
  // SC2: the DATA-GRADIENT of that pair in one pass: gx = dgrad3x3(gy1, w1) + dgrad1x1(gs, ws).  The two gradients are the
  // virtual cat [gy1, gs] along the reduction (DUAL staging, unchanged); the chunks of the second half only run the centre
  // tap, against the 1x1 weights (sc.w) -- +1/9 MFMAs instead of a 1x1 kernel plus an accumulate pass over gx.
  // (F16: both gradients are scaled by ONE power of two, gsc -- smsut_absmax_scale2 -- since they share the accumulators.)
  static_assert(!SC2 || (DUAL && !STATS && !ACC && !BST && !INAFF && !K8 && !SC && KS == 3), "fused shortcut data-gradient");
  static_assert(!(SC2 && F16 && (WINO || N8)), "fused shortcut data-gradient with fp16 operands: the direct form, >= 16 result channels");
  // N8: the result has 8 channels (Ndim == 8: the data-gradient of the first block after the stem, 16 -> 8 @256^2, ran on the per-tile
  // kernel at 35 TFLOP/s).  The weight block is padded to 16 columns with zeros, lanes lm >= 8 neither load nor store.
  static_assert(!N8 || (NTN == 1 && !STATS && !BST && !INAFF && !F16 && !K8 && !SC), "8 result channels: plain / accumulate / SC2 data-gradient forms");
  [[maybe_unused]] const bool nok = !N8 || (threadIdx.x & 15) < 8;
  // F16: fp16 operands (see the block comment above mfma16h, conv_mfma.h); gsc (nullable) = {s, 1/s} for a gradient input.
  // K8: the reduction is 8 channels wide (first block after the stem, network/blocks.py:123-127: 8 -> 16 @256^2).  A 16-wide
  // chunk would be half padding; instead PAIRS OF TAPS share one MFMA: k-slots kq = 0, 1 carry the 8 channels of tap 2g,
  // kq = 2, 3 those of tap 2g+1 (a lane picks its tap's halo offset and weight block) -- 5 x 4 MFMAs per 16x16 output tile
  // instead of 9 x 4.
  static_assert(!K8 || (NCH == 1 && !DUAL && !INAFF && !F16 && !BST), "8-channel reduction: plain / statistics / accumulate / fused-shortcut forms");
  // WINO: Winograd F(2x2, 3x3) (Lavin & Gray 2016) in fp32: 16 element-wise products per 2x2 output tile instead of 36 -- 2.25x
  // fewer MFMAs for the same convolution (the matrix pipes, not HBM, bound this kernel: profiles/r03_step_*_classes.md).  A wave's
  // 4 x 16-pixel output strip is 16 tiles = the MFMA M dimension; lane (lm = tile, kq = channel quad) reads its tile's 4x4 input
  // window from the staged tile, transforms it IN REGISTERS (B^T d B on four channels at once) and the 16 transformed values ARE
  // its A operands of the 16 per-position GEMMs [tiles x Kdim] . [Kdim x 16]; the resident weight block holds U = G g G^T
  // (computed by the workgroup itself from the 3x3 weights); after the last chunk the 16 position accumulators are folded by
  // A^T m A (element-wise over the lane's four tiles) into the SAME accumulator layout the direct form hands to its epilogue --
  // pixel map: acc[i = 2*dy + dx][j][r = tile] = (strip row 2*(kq>>1) + dy, column 8*(kq&1) + 2*r + dx) -- so every fused form (statistics,
  // accumulate, BST, virtual cat, input-side IN, split output) is shared.  Zero padding = the zeroed halo units, as before.
  // Fused shortcut forms under WINO: the 1x1 conv needs the RAW pixels, which the lane holds anyway -- the four output pixels of
  // its tile are window elements (1,1), (1,2), (2,1), (2,2) -- so it is four more MFMA sets per chunk on those (SC, forward);
  // in the data-gradient (SC2) the chunks of the second reduction half (the shortcut's gradient) run ONLY those four sets,
  // against the 1x1 weights, and the result is added after the output transform.
  static_assert(!WINO || (KS == 3 && TH == 16 && !F16 && !K8 && !N8), "Winograd form: 3x3, 16-row items, fp32");
  // O16 (r04, config 5): the result tensor(s) -- y, and sc.y of the fused shortcut -- are stored as fp16 (y points at _Float16
  // [N,H,W,Ndim]): the block-internal raw conv outputs of a BasicBlock cross HBM at half the bytes.  InstanceNorm partials come
  // from the fp32 accumulators, before the rounding.  Forward statistics forms with fp16 operands.
  // With BST (the data-gradient that masks by the block's first InstanceNorm): bst.y1 is such an fp16 tensor; the result stays fp32.
  // (K8 + SC: the first block after the stem, 8 -> 16 -- fp32 operands, its two results stored as fp16 like the other blocks'.)
  static_assert(!O16 || ((F16 || (K8 && SC)) && !ACC && (!INAFF || I16) && (STATS != BST)),
                "fp16 storage: forward statistics forms / BST data-gradient, fp16 operands (or the 8-channel fused-shortcut form)");
  // I16: the INPUT x is such an fp16 tensor (conv2 of a BasicBlock reading the activated a1 another kernel stored as fp16): the
  // staging copies 8-byte units instead of converting 16-byte ones -- the operand bits are those the fp32-input form rounds to.
  // I16 + INAFF: the fp16 input is the RAW conv1 output y1; it is widened, normalised + activated (fp32, as smsut_instnorm_fwd_partials_hs2
  // does) and rounded back while staged -- the a1 tensor and the pass that wrote it disappear, the operand bits stay the same.
  static_assert(!I16 || (F16 && STATS && !BST && !DUAL && !SC), "fp16 input: plain / input-side-IN forward statistics form, fp16 operands");
  constexpr int SPX = WINO ? SPIXW : SPIX;            // pixel stride of the staged fp32 input tile
  constexpr int NPOS = WINO ? 16 : KS * KS;           // weight blocks held in LDS (Winograd positions | taps)
  static_assert(!(BST && (STATS || ACC)), "BST excludes the forward statistics and the accumulate form");
  static_assert(!INAFF || (STATS && !ACC && !BST && !DUAL), "input-side IN: forward statistics form only");
  static_assert(!DUAL || NCH % 2 == 0, "virtual cat input: two equal halves of whole 16-channel chunks");
  // DUAL: the input is the virtual cat([x, x2]) of two [N,H,W,Kdim/2] tensors (common.h): chunks [0, NCH/2) are staged
  // from x, the rest from x2 -- same chunk order, same arithmetic as on the materialised cat.
  constexpr int KST = K8 ? 8 : (DUAL ? 8 * NCH : 16 * NCH);  // pixel stride of the tensor(s) the input is read from
  constexpr int KK = KS * KS;
  constexpr int PAD = (KS - 1) / 2;
  constexpr int IH = TH + KS - 1, IW = TW + KS - 1;
  constexpr int CO_T = 16 * NTN;
  constexpr int MR = TH / 4, NR = NTN;
  constexpr int Kdim = K8 ? 8 : 16 * NCH, K4 = Kdim / 4;
  constexpr int UQ = K8 ? 2 : 4;              // float4 units per pixel of one input chunk
  constexpr int UNITS = IH * IW * UQ;         // float4 units of one input chunk
  constexpr int NI = (UNITS + TPB - 1) / TPB;
  extern __shared__ float smem[];
  float* in_s = smem;                         // [IH][IW][SPIX] + one dummy pixel (sink for the padding units)
  float* red = smem + (IH * IW + 1) * SPX;    // [2][4][CO_T][2] + dummy
  float* w_s = red + 2 * 4 * CO_T * 2 + 8;    // [KK | 16 positions][K4][CO_T][4]
  [[maybe_unused]] float* wsc_s = w_s + NPOS * Kdim * CO_T;           // SC: [K4][CO_T][4]
  [[maybe_unused]] float* red_sc = wsc_s + Kdim * CO_T;               // SC: [2][4][CO_T][2] + dummy
  [[maybe_unused]] _Float16* in_h = reinterpret_cast<_Float16*>(smem);       // F16: [IH][IW][SPIXH] + dummy pixel
  [[maybe_unused]] _Float16* w_h = reinterpret_cast<_Float16*>(w_s);         // F16: [KK][NCH][CO_T][WROWH]
  [[maybe_unused]] _Float16* wsc_h = reinterpret_cast<_Float16*>(wsc_s);     // F16 + SC: [NCH][CO_T][WROWH]
  [[maybe_unused]] const float gs = (F16 && gsc) ? gsc[0] : 1.f, gi = (F16 && gsc) ? gsc[1] : 1.f;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, kq = lane >> 4;
  const int co0 = blockIdx.y * CO_T;
  // split output (y2 != null; plain / accumulate forms only): channels [0, split) of the result live in y with pixel
  // stride `split`, channels [split, Ndim) in y2 with stride Ndim - split -- the data-gradient of a block whose input was
  // cat([up, skip]) lands in the two gradient tensors directly (no split-copy pass).  split % CO_T == 0 (host).
  float* const yo = (y2 && co0 >= split) ? y2 : y;
  const int os = !y2 ? Ndim : (co0 >= split ? Ndim - split : split);      // pixel stride of the tensor this workgroup writes
  const int oc0 = (y2 && co0 >= split) ? co0 - split : co0;
  const int total_items = N * tiles_img;
  // workgroups go to the 8 XCDs round-robin (MICROARCH "Workgroup dispatch"): give XCD k the k-th contiguous eighth of
  // the items, so that the halo rows a strip shares with the strips above / below are hits in that XCD's own L2
  // (PMC: 1.41x -> the algorithmic bytes with the plain mapping, every XCD fetching its neighbours' halos)
  const int wg = (gridDim.x & 7) == 0 ? (int)((blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3)) : (int)blockIdx.x;
  const int item0 = wg * items_per_wg;
  const int item1 = min(item0 + items_per_wg, total_items);
  if (item0 >= item1) return;
  const int tiles_y = tiles_img / tiles_x;
  [[maybe_unused]] const int stamp_wg = blockIdx.y == 0 ? (int)blockIdx.x : -1;
  STAMP(0);

  // ---- resident weights
  if constexpr (WINO) {
    // U = G g G^T per (reduction channel, output channel), G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]; stored like the taps of
    // the direct form with the position in the tap's place: [pos][k4][n][4]
    for (int u = tid; u < Kdim * CO_T; u += TPB) {
      const int n = u % CO_T, ci = u / CO_T;
      const int ng = co0 + n;
      if constexpr (SC2) {                             // second reduction half: the 1x1 weights, parked in position 0's slots
        constexpr int Kh = Kdim / 2;
        if (ci >= Kh) {
          w_s[(((size_t)(ci >> 2)) * CO_T + n) * 4 + (ci & 3)] = sc.w[(size_t)ng * Kh + (ci - Kh)];
          continue;
        }
      }
      constexpr int KROW = SC2 ? Kdim / 2 : Kdim;      // reduction channels of the 3x3 weights proper
      float g[3][3];
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        g[tap / 3][tap % 3] = !(transposed || SC2) ? w[((size_t)tap * Kdim + ci) * Ndim + ng]
                                                   : w[((size_t)(8 - tap) * Ndim + ng) * KROW + ci];
      float t[4][3];
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        t[0][b] = g[0][b];
        t[1][b] = 0.5f * (g[0][b] + g[1][b] + g[2][b]);
        t[2][b] = 0.5f * (g[0][b] - g[1][b] + g[2][b]);
        t[3][b] = g[2][b];
      }
#pragma unroll
      for (int a = 0; a < 4; ++a) {
        const float uu[4] = {t[a][0], 0.5f * (t[a][0] + t[a][1] + t[a][2]), 0.5f * (t[a][0] - t[a][1] + t[a][2]), t[a][2]};
#pragma unroll
        for (int b = 0; b < 4; ++b) w_s[(((size_t)(a * 4 + b) * K4 + (ci >> 2)) * CO_T + n) * 4 + (ci & 3)] = uu[b];
      }
    }
  }
  for (int u = tid; u < (WINO ? 0 : KK * K4 * CO_T); u += TPB) {
    const int n = u % CO_T;
    const int k4 = (u / CO_T) % K4;
    const int tap = u / (CO_T * K4);
    const int ng = co0 + n;
    float4 v;
    if (N8 && n >= 8) {                                  // padding columns of the 8-channel result
      v = make_float4(0.f, 0.f, 0.f, 0.f);
    } else if constexpr (SC2) {                          // (always the transposed form) rows of Kdim/2 = Cout reduction channels
      constexpr int Kh = Kdim / 2;
      if (k4 < K4 / 2) v = *(const float4*)(w + ((size_t)(KK - 1 - tap) * Ndim + ng) * Kh + 4 * k4);
      else if (tap == KK / 2) v = *(const float4*)(sc.w + (size_t)ng * Kh + 4 * (k4 - K4 / 2));
      else v = make_float4(0.f, 0.f, 0.f, 0.f);
    } else if (!transposed) {
      const float* p = w + ((size_t)tap * Kdim + 4 * k4) * Ndim + ng;
      v.x = p[0]; v.y = p[Ndim]; v.z = p[2 * (size_t)Ndim]; v.w = p[3 * (size_t)Ndim];
    } else {
      v = *(const float4*)(w + ((size_t)(KK - 1 - tap) * Ndim + ng) * Kdim + 4 * k4);
    }
    if (F16) *(h4*)(w_h + ((size_t)(tap * NCH + (k4 >> 2)) * CO_T + n) * WROWH + 4 * (k4 & 3)) = to_h4(v);
    else *(float4*)(w_s + (size_t)u * 4) = v;
  }
  if constexpr (SC) {
    for (int u = tid; u < K4 * CO_T; u += TPB) {
      const int n = u % CO_T, k4 = u / CO_T;
      const float* p = sc.w + (size_t)(4 * k4) * Ndim + co0 + n;
      const float4 v = make_float4(p[0], p[Ndim], p[2 * (size_t)Ndim], p[3 * (size_t)Ndim]);
      if (F16) *(h4*)(wsc_h + ((size_t)(k4 >> 2) * CO_T + n) * WROWH + 4 * (k4 & 3)) = to_h4(v);
      else *(float4*)(wsc_s + (size_t)u * 4) = v;
    }
  }

  // ---- per-thread staging descriptors (tile-independent): element offset relative to the tile's first halo pixel,
  //      LDS destination, and which image borders the unit falls outside of (bit 0 top, 1 bottom, 2 left, 3 right)
  int u_off[NI], u_lds[NI], u_flag[NI];
  float4 rin[I16 ? 1 : NI];
  [[maybe_unused]] h4 rinh[I16 ? NI : 1];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int u = tid + i * TPB;
    const bool real = u < UNITS;
    const int uu = real ? u : 0;
    const int q = uu % UQ, pix = uu / UQ;
    const int iy = pix / IW, ix = pix % IW;
    u_off[i] = (iy * W + ix) * KST + 4 * q;
    u_lds[i] = real ? pix * (F16 ? SPIXH : SPX) + 4 * q : IH * IW * (F16 ? SPIXH : SPX);
    u_flag[i] = (iy < PAD ? 1 : 0) | (iy >= TH + PAD ? 2 : 0) | (ix < PAD ? 4 : 0) | (ix >= TW + PAD ? 8 : 0);
  }
  // a unit outside the image reads the tile's first interior pixel instead (always valid) and is zeroed at publish
  const int safe_off = (PAD * W + PAD) * KST;

  // ---- cursors: item being prefetched (p*), item being computed (c*), item whose results are being written (e*)
  int pn = item0 / tiles_img, pty, ptx;
  { const int t = item0 - pn * tiles_img; pty = t / tiles_x; ptx = t - pty * tiles_x; }
  int cn = pn, cty = pty, ctx = ptx;
  int en = pn, ety = pty, etx = ptx;
  int pflags = 0;      // borders the prefetched tile touches
  bool zero[NI];       // per unit: outside the image for the chunk currently in rin
  [[maybe_unused]] float4 a_m, a_r, a_g, a_b;     // INAFF: statistics / affine of (image, this thread's channel quad) for rin

  auto prefetch = [&](int c) __attribute__((always_inline)) {                       // chunk c of item (pn, pty, ptx)
    if (c == 0) pflags = (pty == 0 ? 1 : 0) | (pty == tiles_y - 1 ? 2 : 0) | (ptx == 0 ? 4 : 0) | (ptx == tiles_x - 1 ? 8 : 0);
    const int cl = DUAL ? c % (NCH / 2 > 0 ? NCH / 2 : 1) : c;                          // chunk inside its source tensor
    const int base = (((pn * H + pty * TH - PAD) * W) + ptx * TW - PAD) * KST + cl * 16;   // may be "negative": only
    const float* xb = ((DUAL && c >= NCH / 2) ? x2 : x) + base;                          // used with in-image offsets
    if constexpr (I16) {
      const _Float16* xh = reinterpret_cast<const _Float16*>(x) + base;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        zero[i] = (u_flag[i] & pflags) != 0;
        rinh[i] = *(const h4*)(xh + (zero[i] ? safe_off : u_off[i]));
      }
    } else {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        zero[i] = (u_flag[i] & pflags) != 0;
        rin[i] = *(const float4*)(xb + (zero[i] ? safe_off : u_off[i]));
      }
    }
    if (INAFF) {                                     // every unit of a thread carries the channel quad tid & 3
      const int ch = c * 16 + 4 * (tid & 3);
      a_m = *(const float4*)(aff.mean + (size_t)pn * Kdim + ch);
      a_r = *(const float4*)(aff.rstd + (size_t)pn * Kdim + ch);
      a_g = *(const float4*)(aff.gamma + ch);
      a_b = *(const float4*)(aff.beta + ch);
    }
  };
  auto advance = [&](int& n_, int& ty_, int& tx_) __attribute__((always_inline)) {
    if (++tx_ == tiles_x) { tx_ = 0; if (++ty_ == tiles_y) { ty_ = 0; ++n_; } }
  };
  auto publish = [&]() __attribute__((always_inline)) {
    if constexpr (I16) {
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        h4 hv = rinh[i];
        if constexpr (INAFF) {
          float4 v = make_float4((float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]);
          v.x = aff1(v.x, a_m.x, a_r.x, a_g.x, a_b.x, aff.slope); v.y = aff1(v.y, a_m.y, a_r.y, a_g.y, a_b.y, aff.slope);
          v.z = aff1(v.z, a_m.z, a_r.z, a_g.z, a_b.z, aff.slope); v.w = aff1(v.w, a_m.w, a_r.w, a_g.w, a_b.w, aff.slope);
          hv = to_h4(v);
        }
        *(h4*)(in_h + u_lds[i]) = zero[i] ? (h4){(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f} : hv;
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      float4 v = rin[I16 ? 0 : i];
      if (INAFF) {
        v.x = aff1(v.x, a_m.x, a_r.x, a_g.x, a_b.x, aff.slope); v.y = aff1(v.y, a_m.y, a_r.y, a_g.y, a_b.y, aff.slope);
        v.z = aff1(v.z, a_m.z, a_r.z, a_g.z, a_b.z, aff.slope); v.w = aff1(v.w, a_m.w, a_r.w, a_g.w, a_b.w, aff.slope);
      }
      if (zero[i]) v = make_float4(0.f, 0.f, 0.f, 0.f);          // the zero padding applies to a, not to x
      if (F16) *(h4*)(in_h + u_lds[i]) = to_h4s(v, gs);
      else *(float4*)(in_s + u_lds[i]) = v;
    }
  };

  f32x4 acc[MR][NR], pacc[MR][NR];
  [[maybe_unused]] f32x4 macc[WINO ? 16 : 1][NR];      // WINO: the 16 position accumulators (tiles 4kq..4kq+3, channel lm)
  if constexpr (WINO) {
#pragma unroll
    for (int p_ = 0; p_ < 16; ++p_)
#pragma unroll
      for (int j = 0; j < NR; ++j) macc[p_][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  [[maybe_unused]] f32x4 acs[MR][NR], pacs[MR][NR];    // SC: the shortcut's accumulators (current / previous item)
  [[maybe_unused]] f32x4 qacc[(WINO && (SC || SC2)) ? 4 : 1][NR];   // WINO + SC / SC2: 1x1 products of the tile's four pixels
  if constexpr (WINO && (SC || SC2)) {
#pragma unroll
    for (int q_ = 0; q_ < 4; ++q_)
#pragma unroll
      for (int j = 0; j < NR; ++j) qacc[q_][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  if constexpr (SC) {
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j) { acs[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; pacs[i][j] = acs[i][j]; }
  }
  [[maybe_unused]] f32x4 pold[MR][NR];                 // ACC: what the outputs hold now; BST: y1 at the output positions
  [[maybe_unused]] float nm[NR], nr[NR], ng[NR], nb[NR];   // BST: mean / rstd of (image en, channel), gamma, beta
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) { acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; pacc[i][j] = acc[i][j]; }

  if (BST) {
#pragma unroll
    for (int j = 0; j < NR; ++j) { ng[j] = bst.gamma[co0 + j * 16 + lm]; nb[j] = bst.beta[co0 + j * 16 + lm]; }
  }
  // per-lane output offset of (row wave*MR, col 4*kq, channel lm) inside a tile; red[] slot of this lane
  const int o_lane = WINO ? ((wave * MR + 2 * (kq >> 1)) * W + 8 * (kq & 1)) * os + lm : ((wave * MR) * W + 4 * kq) * os + lm;
  const int red_slot = (wave * CO_T + lm) * 2;
  // pixel of accumulator element (i, r) relative to o_lane, in pixels: direct form row i, column r; Winograd form see above
  auto pxo = [&](int i, int r) __attribute__((always_inline)) { return WINO ? (i >> 1) * W + 2 * r + (i & 1) : i * W + r; };

  // statistics + stores of the item in pacc / (en, ety, etx); straight-line, no branches
  auto epilogue = [&](int par) __attribute__((always_inline)) {
    if (F16) {                                          // undo the gradient-operand scale (1 for forward passes)
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) pacc[i][j] *= gi;
    }
    if (STATS || BST) {
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (BST) {
              const float yv = pold[i][j][r];
              const float gz = pacc[i][j][r] * lrelu_mask(in_affine(yv, nm[j], nr[j], ng[j], nb[j]), bst.slope);
              pacc[i][j][r] = gz;                       // stored below
              s1 += gz; s2 += gz * ((yv - nm[j]) * nr[j]);
            } else {
              const float v = pacc[i][j][r]; s1 += v; s2 += v * v;
            }
          }
        s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
        s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
        float* rd = kq == 0 ? red + par * (4 * CO_T * 2) + j * 32 + red_slot : red + 2 * 4 * CO_T * 2;   // else: dummy slot
        *(float2*)rd = make_float2(s1, s2);
      }
    }
    float* yb = yo + (((size_t)en * H + ety * TH) * W + etx * TW) * os + oc0;
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if constexpr (O16 && !BST) {
            reinterpret_cast<_Float16*>(yo)[(((size_t)en * H + ety * TH) * W + etx * TW) * os + oc0 + o_lane + pxo(i, r) * os + j * 16] =
                (_Float16)pacc[i][j][r];
          } else if (nok) yb[o_lane + pxo(i, r) * os + j * 16] = pacc[i][j][r] + (ACC ? pold[i][j][r] : 0.f);
    if constexpr (SC) {
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) { const float v = pacs[i][j][r]; s1 += v; s2 += v * v; }
        s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
        s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
        float* rd = kq == 0 ? red_sc + par * (4 * CO_T * 2) + j * 32 + red_slot : red_sc + 2 * 4 * CO_T * 2;
        *(float2*)rd = make_float2(s1, s2);
      }
      float* ys = sc.y + (((size_t)en * H + ety * TH) * W + etx * TW) * Ndim + co0;
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if constexpr (O16)
              reinterpret_cast<_Float16*>(sc.y)[(((size_t)en * H + ety * TH) * W + etx * TW) * Ndim + co0 + o_lane + pxo(i, r) * Ndim + j * 16] =
                  (_Float16)pacs[i][j][r];
            else ys[o_lane + pxo(i, r) * Ndim + j * 16] = pacs[i][j][r];
          }
    }
  };
  // ACC: the values the outputs of item (n_, ty_, tx_) hold now (loaded one region before they are added and stored)
  auto load_old = [&](int n_, int ty_, int tx_) __attribute__((always_inline)) {
    if (BST) {
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        nm[j] = bst.mean[(size_t)n_ * Ndim + co0 + j * 16 + lm];
        nr[j] = bst.rstd[(size_t)n_ * Ndim + co0 + j * 16 + lm];
      }
    }
    if (ACC || BST) {
      // (BST never has a split output: os == Ndim, oc0 == co0 there)
      const float* yb = (BST ? bst.y1 : yo) + (((size_t)n_ * H + ty_ * TH) * W + tx_ * TW) * os + oc0;
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if constexpr (BST && O16)
              pold[i][j][r] = (float)reinterpret_cast<const _Float16*>(bst.y1)[(((size_t)n_ * H + ty_ * TH) * W + tx_ * TW) * os + oc0 + o_lane +
                                                                              pxo(i, r) * os + j * 16];
            else pold[i][j][r] = nok ? yb[o_lane + pxo(i, r) * os + j * 16] : 0.f;
          }
    }
  };
  auto stats_out = [&](int par) __attribute__((always_inline)) {                     // after the barrier that completes red[par]
    if ((STATS || BST) && tid < CO_T) {
      const float* rd = red + par * (4 * CO_T * 2);
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int m = 0; m < 4; ++m) { s1 += rd[(m * CO_T + tid) * 2]; s2 += rd[(m * CO_T + tid) * 2 + 1]; }
      float* const po = stats + (((size_t)en * tiles_img + ety * tiles_x + etx) * Ndim + co0 + tid) * 2;
      if constexpr (FIN) st_sc1_f2(po, s1, s2);         // in-launch finalize: write-through, read by the last-arriving workgroup
      else *(float2*)po = make_float2(s1, s2);
      if constexpr (SC) {
        const float* rs = red_sc + par * (4 * CO_T * 2);
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int m = 0; m < 4; ++m) { t1 += rs[(m * CO_T + tid) * 2]; t2 += rs[(m * CO_T + tid) * 2 + 1]; }
        float* const ps = sc.stats + (((size_t)en * tiles_img + ety * tiles_x + etx) * Ndim + co0 + tid) * 2;
        if constexpr (FIN) st_sc1_f2(ps, t1, t2);
        else *(float2*)ps = make_float2(t1, t2);
      }
    }
  };
  auto mma_chunk = [&](int c) __attribute__((always_inline)) {
    if constexpr (WINO) {
      // window of tile (tr, tc) = (lm >> 3, lm & 7) of this wave's strip: rows wave*4 + 2*tr + a, columns 2*tc + b
      const float* dp = in_s + (((wave * 4 + 2 * (lm >> 3)) * IW) + 2 * (lm & 7)) * SPX + 4 * kq;
      const float* wc = w_s + ((size_t)(c * 4 + kq) * CO_T + lm) * 4;
      f32x4 d1[4], d2[4], dx[4];
      if constexpr (SC2) {
        if (c >= NCH / 2) {                           // the shortcut's gradient: 1x1 products of the tile's four pixels only
          const f32x4 px[4] = {*(const f32x4*)(dp + (1 * IW + 1) * SPX), *(const f32x4*)(dp + (1 * IW + 2) * SPX),
                               *(const f32x4*)(dp + (2 * IW + 1) * SPX), *(const f32x4*)(dp + (2 * IW + 2) * SPX)};
#pragma unroll
          for (int j = 0; j < NR; ++j) {
            const f32x4 bw = *(const f32x4*)(wc + (size_t)(j * 16) * 4);
#pragma unroll
            for (int q_ = 0; q_ < 4; ++q_)
#pragma unroll
              for (int s = 0; s < 4; ++s) qacc[q_][j] = mfma16(px[q_][s], bw[s], qacc[q_][j]);
          }
        }
      }
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        dx[b] = *(const f32x4*)(dp + (0 * IW + b) * SPX);
        d1[b] = *(const f32x4*)(dp + (1 * IW + b) * SPX);
        d2[b] = *(const f32x4*)(dp + (2 * IW + b) * SPX);
      }
      if constexpr (SC) {                               // forward shortcut: same four pixels, the 1x1 weights of this chunk
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          const f32x4 bw = *(const f32x4*)(wsc_s + (((size_t)(c * 4 + kq) * CO_T) + j * 16 + lm) * 4);
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            qacc[0][j] = mfma16(d1[1][s], bw[s], qacc[0][j]);
            qacc[1][j] = mfma16(d1[2][s], bw[s], qacc[1][j]);
            qacc[2][j] = mfma16(d2[1][s], bw[s], qacc[2][j]);
            qacc[3][j] = mfma16(d2[2][s], bw[s], qacc[3][j]);
          }
        }
      }
      // (r03: a four-stage software pipeline of this loop -- B-fragment reads and transform arithmetic of row-combination g+1
      //  fenced into the MFMA block of g -- measured no faster at two waves per SIMD, 76.6 vs 77.2 us at 32 x 256^2 16->16, and
      //  cost 28 VGPRs; the other resident wave already covers the LDS latency.  profiles/r03_notes.md)
#pragma unroll
      for (int xi = 0; xi < ((SC2 && c >= NCH / 2) ? 0 : 4); ++xi) {
        if (xi == 3) {
#pragma unroll
          for (int b = 0; b < 4; ++b) dx[b] = *(const f32x4*)(dp + (3 * IW + b) * SPX);
        }
        f32x4 t[4];                                   // row combination xi of B^T: d0-d2 | d1+d2 | d2-d1 | d1-d3
#pragma unroll
        for (int b = 0; b < 4; ++b)
          t[b] = xi == 0 ? sub4(dx[b], d2[b]) : xi == 1 ? add4(d1[b], d2[b]) : xi == 2 ? sub4(d2[b], d1[b]) : sub4(d1[b], dx[b]);
        const f32x4 v[4] = {sub4(t[0], t[2]), add4(t[1], t[2]), sub4(t[2], t[1]), sub4(t[1], t[3])};
#pragma unroll
        for (int nu = 0; nu < 4; ++nu) {
          const int pos = xi * 4 + nu;
#pragma unroll
          for (int j = 0; j < NR; ++j) {
            const f32x4 b = *(const f32x4*)(wc + ((size_t)pos * K4 * CO_T + j * 16) * 4);
#pragma unroll
            for (int s = 0; s < 4; ++s)
              macc[pos][j] = mfma16(v[nu][s], b[s], macc[pos][j]);
          }
        }
      }
      if (c == NCH - 1) {                             // last chunk of the item: A^T m A, element-wise over the lane's four tiles
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          f32x4 c0[4], c1[4];
#pragma unroll
          for (int nu = 0; nu < 4; ++nu) {
            c0[nu] = add4(add4(macc[0 + nu][j], macc[4 + nu][j]), macc[8 + nu][j]);
            c1[nu] = sub4(sub4(macc[4 + nu][j], macc[8 + nu][j]), macc[12 + nu][j]);
          }
          const f32x4 o00 = add4(add4(c0[0], c0[1]), c0[2]), o01 = sub4(sub4(c0[1], c0[2]), c0[3]);
          const f32x4 o10 = add4(add4(c1[0], c1[1]), c1[2]), o11 = sub4(sub4(c1[1], c1[2]), c1[3]);
          // acc[2*dy + dx][j][r] = o[dy][dx][r]: no repacking (the epilogue stores element by element anyway)
          acc[0][j] = o00; acc[1][j] = o01; acc[2][j] = o10; acc[3][j] = o11;
#pragma unroll
          for (int p_ = 0; p_ < 16; ++p_) macc[p_][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
          if constexpr (SC || SC2) {                   // the 1x1 products in the same pixel map (qacc[2*dy + dx][j][r])
            if constexpr (SC) { acs[0][j] = qacc[0][j]; acs[1][j] = qacc[1][j]; acs[2][j] = qacc[2][j]; acs[3][j] = qacc[3][j]; }
            else { acc[0][j] += qacc[0][j]; acc[1][j] += qacc[1][j]; acc[2][j] += qacc[2][j]; acc[3][j] += qacc[3][j]; }
#pragma unroll
            for (int q_ = 0; q_ < 4; ++q_) qacc[q_][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
          }
        }
      }
      return;
    }
    if constexpr (K8) {
      const int half = kq >> 1, kk = kq & 1;
#pragma unroll
      for (int g = 0; g < (KK + 1) / 2; ++g) {
        constexpr int dummy = 0; (void)dummy;
        const int tA = 2 * g, tB = (2 * g + 1 < KK) ? 2 * g + 1 : 2 * g;      // (the unpaired last tap: second half zeroed)
        const int t = half ? tB : tA;
        const bool live = !(half && 2 * g + 1 >= KK);
        const int toff = ((t / KS) * IW + (t % KS)) * SPIX + 4 * kk;
        f32x4 a[MR], b[NR];
#pragma unroll
        for (int i = 0; i < MR; ++i) a[i] = *(const f32x4*)(in_s + ((wave * MR + i) * IW + lm) * SPIX + toff);
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          b[j] = *(const f32x4*)(w_s + (((size_t)(t * K4 + kk) * CO_T) + j * 16 + lm) * 4);
          if (!live) b[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int i = 0; i < MR; ++i)
#pragma unroll
            for (int j = 0; j < NR; ++j) acc[i][j] = mfma16(a[i][s], b[j][s], acc[i][j]);
        if constexpr (SC) {
          if (2 * g == KK / 2) {                           // this group's first half is the centre tap: the 1x1 shortcut rides on it
            f32x4 bs[NR];                                  // (k-slots of the second half, tap 5, multiply zeros)
#pragma unroll
            for (int j = 0; j < NR; ++j) {
              bs[j] = *(const f32x4*)(wsc_s + (((size_t)kk * CO_T) + j * 16 + lm) * 4);
              if (half) bs[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
              for (int i = 0; i < MR; ++i)
#pragma unroll
                for (int j = 0; j < NR; ++j) acs[i][j] = mfma16(a[i][s], bs[j][s], acs[i][j]);
          }
        }
      }
      return;
    }
    if constexpr (F16 && SMSUT_F16_X32) {
      // tap pairs on the 32-deep instruction (comment at mfma32h); lone taps multiply zeros in the upper sixteen k-slots
      const bool sc2_half = SC2 && c >= NCH / 2;
      const bool hi = kq >= 2;
      const int ko = 8 * (kq & 1);
      const h8 zero8 = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
#pragma unroll
      for (int p = 0; p < (KK + 1) / 2; ++p) {
        if (sc2_half && p != (KK / 2) / 2) continue;            // the shortcut's gradient: centre tap only
        const bool solo = 2 * p + 1 >= KK || sc2_half;          // no second tap in this issue
        const int tlo = sc2_half ? KK / 2 : 2 * p, thi = (2 * p + 1 < KK) ? 2 * p + 1 : 2 * p;
        const int tap = hi ? thi : tlo;
        const int kh = hi ? thi / KS : tlo / KS, kw = hi ? thi % KS : tlo % KS;
        h8 a[MR], b[NR];
#pragma unroll
        for (int i = 0; i < MR; ++i) {
          a[i] = *(const h8*)(in_h + ((wave * MR + i + kh) * IW + lm + kw) * SPIXH + ko);
          if (solo && hi) a[i] = zero8;
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          b[j] = *(const h8*)(w_h + ((size_t)(tap * NCH + c) * CO_T + j * 16 + lm) * WROWH + ko);
          if (solo && hi) b[j] = zero8;
        }
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < NR; ++j) acc[i][j] = mfma32h(a[i], b[j], acc[i][j]);
        if constexpr (SC) {
          if (2 * p == KK / 2 || 2 * p + 1 == KK / 2) {    // the pair that holds the centre tap: the 1x1 shortcut rides on that half
            const bool mine = hi == (2 * p + 1 == KK / 2); // (the other half's k-slots multiply zeros)
            h8 bs[NR];
#pragma unroll
            for (int j = 0; j < NR; ++j) {
              bs[j] = *(const h8*)(wsc_h + ((size_t)c * CO_T + j * 16 + lm) * WROWH + ko);
              if (!mine) bs[j] = zero8;
            }
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
              for (int j = 0; j < NR; ++j) acs[i][j] = mfma32h(a[i], bs[j], acs[i][j]);
          }
        }
      }
      return;
    }
    if constexpr (F16) {
#pragma unroll
      for (int tap = 0; tap < KK; ++tap) {
        if (SC2 && c >= NCH / 2 && tap != KK / 2) continue;     // the shortcut's gradient: centre tap only
        const int kh = tap / KS, kw = tap % KS;
        h4 a[MR], b[NR];
#pragma unroll
        for (int i = 0; i < MR; ++i)
          a[i] = *(const h4*)(in_h + ((wave * MR + i + kh) * IW + lm + kw) * SPIXH + 4 * kq);
#pragma unroll
        for (int j = 0; j < NR; ++j)
          b[j] = *(const h4*)(w_h + ((size_t)(tap * NCH + c) * CO_T + j * 16 + lm) * WROWH + 4 * kq);
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < NR; ++j) acc[i][j] = mfma16h(a[i], b[j], acc[i][j]);
        if constexpr (SC) {
          if (tap == KK / 2) {                             // the 1x1 shortcut (r04, config 5): centre tap, its own weights, same A fragments
            h4 bs[NR];
#pragma unroll
            for (int j = 0; j < NR; ++j) bs[j] = *(const h4*)(wsc_h + ((size_t)c * CO_T + j * 16 + lm) * WROWH + 4 * kq);
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
              for (int j = 0; j < NR; ++j) acs[i][j] = mfma16h(a[i], bs[j], acs[i][j]);
          }
        }
      }
      return;
    }
    const float* wc = w_s + (size_t)(c * 4) * CO_T * 4;
#pragma unroll
    for (int tap = 0; tap < KK; ++tap) {
      if (SC2 && c >= NCH / 2 && tap != KK / 2) continue;       // the shortcut's gradient: centre tap only
      const int kh = tap / KS, kw = tap % KS;
      const int tapw = tap;
      f32x4 a[MR], b[NR];
#pragma unroll
      for (int i = 0; i < MR; ++i)
        a[i] = *(const f32x4*)(in_s + ((wave * MR + i + kh) * IW + lm + kw) * SPIX + 4 * kq);
#pragma unroll
      for (int j = 0; j < NR; ++j)
        b[j] = *(const f32x4*)(wc + (((size_t)(tapw * K4 + kq) * CO_T) + j * 16 + lm) * 4);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < NR; ++j) acc[i][j] = mfma16(a[i][s], b[j][s], acc[i][j]);
      if constexpr (SC) {
        if (tap == KK / 2) {                             // the 1x1 shortcut: centre tap, its own weights, same A fragments
          f32x4 bs[NR];
#pragma unroll
          for (int j = 0; j < NR; ++j) bs[j] = *(const f32x4*)(wsc_s + (((size_t)(c * 4 + kq) * CO_T) + j * 16 + lm) * 4);
#pragma unroll
          for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < MR; ++i)
#pragma unroll
              for (int j = 0; j < NR; ++j) acs[i][j] = mfma16(a[i][s], bs[j][s], acs[i][j]);
        }
      }
    }
  };

  STAMP(1);
  load_old(cn, cty, ctx);
  prefetch(0);
  if (NCH == 1) advance(pn, pty, ptx);
  __syncthreads();                                    // (also publishes w_s)
  publish();
  __syncthreads();
  STAMP(2);
  int par = 0;
  // one item = NCH regions; FIRST (compile-time) drops the previous-item epilogue from the workgroup's first item
  auto item_body = [&](int item, auto first_tag) __attribute__((always_inline)) {
    constexpr bool FIRST = decltype(first_tag)::value;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      // ---- one straight-line region: next loads, previous item's results, this chunk's MFMAs
      const bool more = c + 1 < NCH || item + 1 < item1;
      if (more) {
        prefetch((c + 1) % NCH);
        if (c + 2 == NCH || (NCH == 1)) advance(pn, pty, ptx);     // the prefetch after the next one starts a new item
      }
      if (c == 0 && !FIRST) {
        epilogue(par);
        load_old(cn, cty, ctx);
      }
      mma_chunk(c);
      if (item == item0 + 1 && c < 2) { STAMP(3 + 4 * c); }
      __syncthreads();                                // in_s is free; red[par] is complete
      if (item == item0 + 1 && c < 2) { STAMP(4 + 4 * c); }
      if (c == 0 && !FIRST) { stats_out(par); par ^= 1; }
      if (more) publish();
      if (item == item0 + 1 && c < 2) { STAMP(5 + 4 * c); }
      __syncthreads();
      if (item == item0 + 1 && c < 2) { STAMP(6 + 4 * c); }
    }
    // item done: keep its accumulators for the next region's epilogue
#pragma unroll
    for (int i = 0; i < MR; ++i)
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        pacc[i][j] = acc[i][j]; acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if constexpr (SC) { pacs[i][j] = acs[i][j]; acs[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
      }
    en = cn; ety = cty; etx = ctx;
    advance(cn, cty, ctx);
  };
  item_body(item0, std::true_type{});
  for (int item = item0 + 1; item < item1; ++item) item_body(item, std::false_type{});
  epilogue(par);
  if (STATS || BST) { __syncthreads(); stats_out(par); }
  if constexpr (FIN)                                    // the image(s) this workgroup completes: finalised here
    fin_tail<!BST>(fin, stats, SC ? sc.stats : nullptr, item0, item1, tiles_img, tiles_img * (int)gridDim.y, Ndim, H * W,
                   reinterpret_cast<int*>(smem + 1024), reinterpret_cast<double*>(smem));
  STAMP(11);
}

template <int KS, int TH, int WM, int WN, int NTN, int MW = TW>
int launch_fwd(const ConvCall& c) {
  constexpr int IH = TH + KS - 1, IW = MW + KS - 1;
  constexpr size_t sh16 = (size_t)(IH * IW * SPIX + KS * KS * CK * 16 * NTN) * sizeof(float);
  // (fp16 operands in 32-channel passes: the weight image [taps][16 NTN][40 halves] starts where the fp32 one would)
  constexpr size_t sh32 = (size_t)(IH * IW * SPIX) * sizeof(float) + (size_t)(KS * KS * 16 * NTN * 40) * sizeof(_Float16);
  constexpr size_t sh = sh16;
  static_assert(sh16 <= 64 * 1024 && (KS != 3 || MW != TW || sh32 <= 64 * 1024), "LDS budget");
  const int tiles_x = (c.W + MW - 1) / MW, tiles_y = (c.H + TH - 1) / TH;
  const bool plain_taps = c.isc == 1 && c.osc == 1 && c.G == 1 && c.ntap_out == 1;
  if (MW != TW && !plain_taps) return -1;
  const int nz = (c.Ndim + 16 * NTN - 1) / (16 * NTN);
  if (c.tiles_out) { *c.tiles_out = tiles_x * tiles_y; return 0; }          // planning query only
  dim3 grid(tiles_x * tiles_y, c.N, nz * c.ntap_out);
  if ((c.x2 && (!plain_taps || c.transposed_w || c.Kdim % 32 != 0)) ||
      (c.y2 && (c.osc != 1 || c.ntap_out != 1 || c.stats || c.split <= 0 || c.split >= c.Ndim || c.split % 16 != 0)))
    return -1;
  auto go = [&](auto kern, size_t lds) {             // (this kernel's operands are fp32 tensors)
    kern<<<grid, TPB, lds, c.stream>>>((const float*)c.x, c.w, (float*)c.y, c.H, c.W, c.Kdim, c.Ndim, tiles_x, c.transposed_bits(), c.isc,
                                       c.osc, c.G, nz, c.stats, c.x2, c.y2, c.split, c.gsc);
    return 0;
  };
  if constexpr (KS == 3 && MW == TW && SMSUT_F16_X32) {
    // 32-channel passes on every tile shape (config 5: 49.50 ms with 16-channel passes -> 48.56 ms, 48.95 with 32-channel passes on
    // the 16-row tiles only)
    if (c.f16_operands && c.Kdim % 32 == 0 && c.Kdim >= 32 && (!c.x2 || (c.Kdim / 2) % 32 == 0) && c.isc == 1 && c.osc == 1 && c.G == 1)
      return go(conv_mfma_fwd<KS, TH, WM, WN, NTN, true, MW, 32>, sh32);
  }
  if (c.f16_operands) return go(conv_mfma_fwd<KS, TH, WM, WN, NTN, true, MW>, sh);
  return go(conv_mfma_fwd<KS, TH, WM, WN, NTN, false, MW>, sh);
}

// Persistent variant: LDS bytes and eligibility (see conv_mfma_fwd_p).
template <int KS, int TH, int NTN, int NCH, bool WINO = false>
constexpr size_t fwd_p_lds() {
  return (size_t)(((TH + KS - 1) * (TW + KS - 1) + 1) * (WINO ? SPIXW : SPIX) + 2 * 4 * 16 * NTN * 2 + 8 +
                  (WINO ? 16 : KS * KS) * 16 * NCH * 16 * NTN) * sizeof(float);
}


// resident workgroups per CU of ONE kernel instantiation at the dynamic LDS size it is launched with (which is a function of its
// template arguments, so one query per instantiation; magic static: safe under concurrent host threads)
template <auto Kern>
inline int p_occupancy(size_t lds) {
  static const int occ = [lds] {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    int o = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, Kern, TPB, lds) != hipSuccess || o < 1) o = 1;
    return o;
  }();
  return occ;
}

// Launch sites name a form by its F_* bits (common.h): fwd_p_kernel<KS, TH, NTN, NCH, F_STATS | F_SC | F_K8> is that instantiation
// of conv_mfma_fwd_p.  The kernel's own parameter list stays one bool per flag, in this order: the roofline legs of bench.py and
// profiles/summarize.py find a kernel in a trace by that list.
template <int KS, int TH, int NTN, int NCH, unsigned F>
constexpr auto fwd_p_kernel =
    conv_mfma_fwd_p<KS, TH, NTN, NCH, (F & F_STATS) != 0, (F & F_ACC) != 0, (F & F_BST) != 0, (F & F_DUAL) != 0, (F & F_INAFF) != 0,
                    (F & F_F16) != 0, (F & F_K8) != 0, (F & F_SC) != 0, (F & F_SC2) != 0, (F & F_N8) != 0, (F & F_WINO) != 0,
                    (F & F_O16) != 0, (F & F_I16) != 0, (F & F_FIN) != 0>;

template <int KS, int TH, int NTN, int NCH, bool K8 = false, bool N8 = false, bool WINO = false>
int launch_fwd_p(const ConvCall& c) {
  const bool tw = c.transposed_w, acc = c.accumulate, f16 = c.f16_operands, o16 = c.out_f16, i16 = c.in_f16;
  const auto x2 = c.x2; const auto y2 = c.y2; const auto stats = c.stats;
  const auto bst = c.bst; const auto aff = c.aff; const auto sc = c.sc; const auto fin = c.fin;
  const int N = c.N, H = c.H, W = c.W, Kdim = c.Kdim, Ndim = c.Ndim, split = c.split;
  // in-launch finalize (FIN instantiations): fp32 statistics / BST forms of the fused block -- plain, input-side IN, fused shortcut
  if (fin && (!fin->tickets || !fin->o0 || !fin->o1 || !stats || f16 || N8 || y2 || o16 || i16 || acc ||
              (fin->s0 && !(sc && !tw && sc->stats && fin->s1)) || (!fin->s0 && sc)))
    return -1;
  constexpr size_t sh = fwd_p_lds<KS, TH, NTN, NCH, WINO>();
  // fused 1x1 shortcut (SC): its weight block and a second statistics scratch
  constexpr size_t sh_sc = sh + (size_t)(16 * NCH * 16 * NTN + 2 * 4 * 16 * NTN * 2 + 8) * sizeof(float);
  if constexpr (sh > (WINO ? 160 : 64) * 1024) return -1;
  else {
  if (Kdim != (K8 ? 8 : 16 * NCH) || W % TW != 0 || H % TH != 0 || (N8 ? Ndim != 8 : Ndim % (16 * NTN) != 0) ||
      (int64_t)N * H * W * (Kdim > Ndim ? Kdim : Ndim) >= (1ll << 31))
    return -1;
  if (N8 && (NTN != 1 || K8 || stats || c.tiles_out || bst || y2 || aff || f16 || !tw || (x2 && !(sc && sc->w)))) return -1;
  if (K8 && (f16 || bst || x2 || aff)) return -1;
  if (WINO && (f16 || K8 || N8)) return -1;                                    // Winograd form: fp32
  const int tiles_x = W / TW, tiles_y = H / TH;
  const int tiles_img = tiles_x * tiles_y;
  if (y2 && (split <= 0 || split >= Ndim || split % (16 * NTN) != 0 || stats || bst)) return -1;
  if (x2 && !(sc && tw) && (NCH % 2 != 0 || !stats || bst || y2 || tw || acc)) return -1;   // virtual-cat input: forward statistics form
  if (aff && (!stats || bst || y2 || x2 || tw || acc)) return -1;                // input-side IN: forward statistics form
  const bool sc2 = sc && tw;                                                    // fused shortcut DATA-gradient (see SC2)
  if (sc2 && (K8 || KS != 3 || NCH % 2 != 0 || !x2 || stats || bst || aff || acc || (f16 && (WINO || N8)) || !sc->w)) return -1;
  if (sc && !sc2 && (KS != 3 || sh_sc > 64 * 1024 || !stats || bst || y2 || aff || tw || acc || !sc->w || !sc->y || !sc->stats ||
                     (K8 && x2) || (f16 && (K8 || WINO))))
    return -1;                                                                  // fused shortcut: forward statistics forms
  if (i16 && (!o16 || bst || x2 || sc)) return -1;
  if (o16 && !bst && (!(f16 || (K8 && sc)) || !stats || (aff && !i16) || y2 || tw || acc || (K8 && !sc) || N8 || WINO || KS != 3)) return -1;   // fp16 result storage
  if (o16 && bst && (!f16 || !stats || aff || y2 || x2 || sc || acc || K8 || N8 || WINO || KS != 3)) return -1;  // fp16 y1 of the BST form
  if (c.tiles_out) { *c.tiles_out = tiles_img; return 0; }
  const int nz = N8 ? 1 : Ndim / (16 * NTN);
  // The persistent grid is sized for ONE resident round of the kernel instantiation ACTUALLY launched, at its own dynamic LDS size
  // (go below; ADVICE r04: one occupancy figure -- the fp32 statistics form's -- used to serve every form of this template, whatever
  // its registers and LDS: fused shortcut, fp16 operands, half storage).
  const int64_t items = (int64_t)N * tiles_img;
  int ipw = 1;
  dim3 grid(1, nz);
  auto size_grid = [&](int occ) {
    const int64_t slots = (int64_t)device_cus() * occ;
    ipw = (int)((items * nz + slots - 1) / slots);        // one resident round: each workgroup walks ipw consecutive items
    if (ipw < 1) ipw = 1;
    grid.x = (unsigned)((items + ipw - 1) / ipw);
  };
  // one launch site for every form.  The fp16 buffers of the half-storage forms (x, y) travel as the kernel's float pointers.
  auto go = [&](auto form, size_t lds) {
    constexpr auto kern = fwd_p_kernel<KS, TH, NTN, NCH, decltype(form)::value>;
    size_grid(p_occupancy<kern>(lds));
    kern<<<grid, TPB, lds, c.stream>>>((const float*)c.x, c.w, (float*)c.y, N, H, W, Ndim, tiles_x, tiles_img, ipw, tw ? 1 : 0, stats,
                                       bst ? *bst : BstRef{}, y2, split, x2, aff ? *aff : AffRef{}, f16 ? c.gsc : nullptr,
                                       sc ? *sc : ScRef{}, fin ? *fin : FinRef{});
    return 0;
  };
  // `form`, with the bits of `extra` when `on`: a run-time twin, both of which this instantiation has
  auto go_opt = [&](bool on, auto extra, auto form, size_t lds) {
    return on ? go(Form<decltype(form)::value | decltype(extra)::value>{}, lds) : go(form, lds);
  };
  // the plain family (statistics, accumulate, BST, virtual cat, input-side IN) in this instantiation's arithmetic (K8 / WINO / direct),
  // with the in-launch finalize or the fp16-operand twin chosen at run time
  auto go_plain = [&](auto form) {
    constexpr unsigned B = decltype(form)::value | (K8 ? F_K8 : 0u) | (WINO ? F_WINO : 0u);
    if constexpr (K8 && (B & (F_BST | F_DUAL | F_INAFF)) != 0) return -1;
    else {
      if constexpr ((B & (F_STATS | F_BST)) != 0 && !(B & F_ACC)) {
        if (fin) return go(Form<B | F_FIN>{}, sh);          // the same form, finalising its statistics in the launch
      }
      if constexpr (!K8 && !WINO) return go_opt(f16, Form<F_F16>{}, Form<B>{}, sh);
      else return go(Form<B>{}, sh);
    }
  };
  // (every `if constexpr` below ends in `else return -1`: a form this instantiation does not have must report
  //  "nothing launched", never fall through to `return 0` with y / ysc / the statistics left unwritten)
  if constexpr (N8) {                           // 8 result channels: data-gradient forms only (checked above)
    if constexpr (NTN == 1 && !K8 && KS == 3) {
      if (sc2) {
        if constexpr (NCH % 2 == 0) return go(Form<F_DUAL | F_SC2 | F_N8>{}, sh);
        else return -1;
      }
      return go_opt(acc, Form<F_ACC>{}, Form<F_N8>{}, sh);
    } else return -1;
  } else if (sc2) {
    if constexpr (!K8 && KS == 3 && NCH % 2 == 0) {
      if (f16) {
        if constexpr (!WINO) return go(Form<F_DUAL | F_F16 | F_SC2>{}, sh);
        else return -1;
      }
      return go(Form<F_DUAL | F_SC2 | (WINO ? F_WINO : 0u)>{}, sh);
    } else return -1;
  } else if (sc) {
    if constexpr (K8 && KS == 3 && sh_sc <= 64 * 1024) {
      if (o16) return go(Form<F_STATS | F_K8 | F_SC | F_O16>{}, sh_sc);
      return go_opt(fin != nullptr, Form<F_FIN>{}, Form<F_STATS | F_K8 | F_SC>{}, sh_sc);
    } else if constexpr (!K8 && KS == 3 && sh_sc <= 64 * 1024) {
      if (f16) {                                   // fp16 operands (config 5; r04): direct form, plain or virtual-cat input
        if constexpr (!WINO) {
          if (!x2) return go_opt(o16, Form<F_O16>{}, Form<F_STATS | F_F16 | F_SC>{}, sh_sc);
          if constexpr (NCH % 2 == 0) return go_opt(o16, Form<F_O16>{}, Form<F_STATS | F_DUAL | F_F16 | F_SC>{}, sh_sc);
          else return -1;
        } else return -1;
      }
      constexpr unsigned SCW = F_STATS | F_SC | (WINO ? F_WINO : 0u);
      if (!x2) return go_opt(fin != nullptr, Form<F_FIN>{}, Form<SCW>{}, sh_sc);
      if constexpr (NCH % 2 == 0) return go_opt(fin != nullptr, Form<F_FIN>{}, Form<SCW | F_DUAL>{}, sh_sc);
      else return -1;
    } else return -1;
  } else if (aff && i16) {                        // fp16 y1 in, normalised while staged, fp16 y2 out (half-storage conv2)
    if constexpr (!K8 && !WINO && KS == 3) return go(Form<F_STATS | F_INAFF | F_F16 | F_O16 | F_I16>{}, sh);
    else return -1;
  } else if (aff) {
    return go_plain(Form<F_STATS | F_INAFF>{});
  } else if (o16 && !bst) {                       // fp16 operands, fp16 result storage: plain or virtual-cat forward statistics form
    if constexpr (!K8 && !WINO && KS == 3) {
      if (!x2) return go_opt(i16, Form<F_I16>{}, Form<F_STATS | F_F16 | F_O16>{}, sh);
      if constexpr (NCH % 2 == 0) return go(Form<F_STATS | F_DUAL | F_F16 | F_O16>{}, sh);
      else return -1;
    } else return -1;
  } else if (x2) {
    if constexpr (NCH % 2 == 0) return go_plain(Form<F_STATS | F_DUAL>{});
    else return -1;
  } else if (bst && o16) {
    if constexpr (!K8 && !WINO && KS == 3) return go(Form<F_BST | F_F16 | F_O16>{}, sh);
    else return -1;
  } else if (bst) {
    if (!stats || acc) return -1;
    return go_plain(Form<F_BST>{});
  } else if (acc) {
    if (stats) return -1;
    return go_plain(Form<F_ACC>{});
  } else if (stats) return go_plain(Form<F_STATS>{});
  else return go_plain(Form<0u>{});
  }
}

// shapes the persistent kernel takes (3x3 regular conv): resident weight block fits, full tiles, enough items to fill
// one resident round
inline bool fwd_p_eligible(int N, int H, int W, int Kdim, int Ndim) {
  return (Kdim == 8 || Kdim == 16 || Kdim == 32 || Kdim == 64) && W % TW == 0 && H % 8 == 0 && Ndim % 16 == 0 &&
         (int64_t)N * (H / 8) * (W / TW) * (Ndim / 16) >= 1024 && (int64_t)N * H * W * (Kdim > Ndim ? Kdim : Ndim) < (1ll << 31);
}

// ... or the large-reduction Winograd kernel (conv_wino.hip: fp32 only, Kdim >= 64, 16x16 tiles)
constexpr int WINO_L_MIN_K = 64;
inline bool wino_l_shape(int N, int H, int W, int Kdim, int Ndim) {
  return winograd_on() && Kdim >= WINO_L_MIN_K && smsut_wino_l_eligible(N, H, W, Kdim, Ndim);
}
inline bool fwd_any_eligible(int N, int H, int W, int Kdim, int Ndim, bool f16) {
  return fwd_p_eligible(N, H, W, Kdim, Ndim) || (!f16 && wino_l_shape(N, H, W, Kdim, Ndim));
}

// Variant table of the persistent kernel, from the late-r01 sweep (scratch/bench_conv.py 32: cfg 20..29 on the U-Net
// shapes, forward and data-gradient): 16-channel reductions run ~10 % faster on 16-row items (109 vs 99 TF at 256^2
// 16->16, 103 vs 88 at 128^2 16->32), 32-channel reductions ~8 % faster with 32 output channels per workgroup when
// Ndim allows it (120 vs 111 TF at 128^2 32->32).  ONE selector for the plain, statistics, accumulate and BST forms,
// so that smsut_conv2d_mfma_tiles() always describes the partials the launched variant writes.
inline int select_fwd_p(const ConvCall& c) {
  const int N = c.N, H = c.H, W = c.W, Kdim = c.Kdim, Ndim = c.Ndim;
  const bool f16 = c.f16_operands;
  // (the fused shortcut data-gradient at 64 reduction channels stays on the direct resident-weight form: 107 us vs 142 us at
  //  16 x 128^2 (32 + 32) -> 64 -- its second-half chunks are a run-time branch inside the staging parts, r03 notes)
  const bool sc2_64 = c.sc && c.transposed_w && Kdim == 64 && fwd_p_eligible(N, H, W, Kdim, Ndim);
  if (!f16 && !sc2_64 && wino_l_shape(N, H, W, Kdim, Ndim)) return smsut_wino_l_launch(c);   // Winograd, streamed weights (conv_wino.hip): every fp32 form
  if (Ndim == 8) {                                   // 8 result channels (see conv_mfma_fwd_p, N8): data-gradient forms
    if (Kdim == 16) return (H % 16 == 0) ? launch_fwd_p<3, 16, 1, 1, false, true>(c) : launch_fwd_p<3, 8, 1, 1, false, true>(c);
    if (Kdim == 32) return launch_fwd_p<3, 8, 1, 2, false, true>(c);   // (16-row items measured no better: 8.89 vs 8.91 ms U-Net)
    return -1;
  }
  if (Kdim == 8) return (H % 16 == 0) ? launch_fwd_p<3, 16, 1, 1, true>(c) : launch_fwd_p<3, 8, 1, 1, true>(c);
  // Winograd F(2x2,3x3) form (r03: 1.2-1.4x the direct form on these shapes, scratch/wino_probe.py): every fp32 form of the
  // 16- and 32-channel reductions on 16-row items (winograd_on(): the direct forms are the reference).  Chosen by SHAPE only,
  // never by form, so that the forms of one shape stay bit-identical to each other (virtual cat vs materialised, fused shortcut vs
  // plain, input-side IN vs applied).
  if (winograd_on() && !f16 && H % 16 == 0 && (Kdim == 16 || Kdim == 32))
    return Kdim == 16 ? launch_fwd_p<3, 16, 1, 1, false, false, true>(c) : launch_fwd_p<3, 16, 1, 2, false, false, true>(c);
  if (Kdim == 16 && H % 16 == 0) return launch_fwd_p<3, 16, 1, 1>(c);
  // (fp16 operands, Kdim 32 stay on 8-row items: 16-row items re-read 1.27x their input as halo instead of 1.41x, but the halo rows
  //  are L2 hits under the XCD-aware item map -- config 5 measured 52.77 ms on 8-row items, 52.80 with 16-row items for Ndim 16 only,
  //  53.59 with them on every Kdim-32 shape)
  if (Kdim == 32 && Ndim % 32 == 0 && !(c.y2 && c.split % 32 != 0)) return launch_fwd_p<3, 8, 2, 2>(c);   // (32-channel slabs must not straddle a split)
  if (Kdim == 16) return launch_fwd_p<3, 8, 1, 1>(c);
  if (Kdim == 32) return launch_fwd_p<3, 8, 1, 2>(c);
  if (Kdim == 64) return launch_fwd_p<3, 8, 1, 4>(c);
  return -1;
}

// 8-channel results on the persistent kernel (data-gradient of the first block after the stem)
inline bool fwd_p_n8_eligible(int N, int H, int W, int Kdim, int Ndim) {
  return Ndim == 8 && (Kdim == 16 || Kdim == 32) && W % TW == 0 && H % 8 == 0 && (int64_t)N * (H / 8) * (W / TW) >= 1024 &&
         (int64_t)N * H * W * Kdim < (1ll << 31);
}

template <int KS>
int dispatch_fwd(const ConvCall& c) {
  const int N = c.N, H = c.H, W = c.W, Kdim = c.Kdim, Ndim = c.Ndim;
  const bool plain_taps = c.isc == 1 && c.osc == 1 && c.G == 1 && c.ntap_out == 1;
  // From the r01 sweep (scratch/bench_conv.py, B=32, U-Net shapes): 8-row tiles win everywhere; 32 output channels
  // per workgroup (grid.z walks the rest) beat 64, and 16 win when the grid would otherwise be < ~4 WGs per CU.
  if constexpr (KS == 3) {
    // small-Cin / large-image layers: persistent kernel with resident weights (see conv_mfma_fwd_p); it declines
    // (-1) shapes it does not cover, which fall through to the per-tile kernel below.
    if (plain_taps && fwd_any_eligible(N, H, W, Kdim, Ndim, c.f16_operands)) {
      if (select_fwd_p(c) == 0) return 0;
    }
    if (plain_taps && c.transposed_w && !c.stats && !c.tiles_out && !c.x2 && !c.y2 && !c.f16_operands &&
        fwd_p_n8_eligible(N, H, W, Kdim, Ndim)) {
      if (select_fwd_p(c) == 0) return 0;
    }
  }
  const int nt = (Ndim + 15) / 16;
  const int tx = (W + TW - 1) / TW;
  const int64_t wg16 = (int64_t)tx * ((H + 15) / 16) * N * ((nt + 1) / 2) * c.ntap_out;
  const int64_t wg8 = (int64_t)tx * ((H + 7) / 8) * N * ((nt + 1) / 2) * c.ntap_out;
  // planes of <= 4 rows (discriminator 4x4 level): the 4-row tile halves the rows of padding every MFMA multiplies --
  // scratch/bench_conv_small.py, 256->256: 19.4 vs 29.1 us forward, 25.1 vs 32.7 us data-gradient at B=16 (28.7 vs 48.2 at 32)
  // 8x8 planes of the discriminator's deep levels: M-tiles of real pixels only -- four (2 rows x 8 columns) tiles per plane, 16
  // output channels per workgroup so that B=16 still gives one workgroup per CU.
  // (4x4 planes stay on the 4-row tile: a plane is ONE M-tile, and 64-channel workgroups leave 64 of them for 256 CUs --
  //  measured 71 us vs 19-25 us; there the limit is parallelism, not padded MFMAs.)
  if (plain_taps && !c.f16_operands && H <= 8 && W <= 8 && H > 4) return launch_fwd<KS, 8, 4, 1, 1, 8>(c);
  if (H <= 4 && c.isc == 1 && c.osc == 1) return launch_fwd<KS, 4, 4, 1, 1>(c);
  if (nt == 1) return launch_fwd<KS, 8, 4, 1, 1>(c);
  if (wg16 >= 512) return launch_fwd<KS, 16, 4, 1, 2>(c);       // >= 2 workgroups per CU with the big tile
  // mid-size grids: 32 output channels per workgroup for the forward form; the data-gradient form (float4 weight rows)
  // runs 10-17 % faster with 16 (same sweep: 51.3 vs 60.0 us at 16x16 256->256, 49.4 vs 59.3 us at B32 8x8)
  if (wg8 >= 256 && !c.transposed_w) return launch_fwd<KS, 8, 4, 1, 2>(c);
  return launch_fwd<KS, 8, 4, 1, 1>(c);
}

// tuning hook: force a tile configuration (scratch/bench_conv.py sweeps these to fill dispatch_fwd's table)
template <int KS>
int dispatch_fwd_cfg(int cfg, const ConvCall& c) {
  switch (cfg) {
    case 0: return launch_fwd<KS, 16, 4, 1, 1>(c);
    case 1: return launch_fwd<KS, 8, 4, 1, 1>(c);
    case 2: return launch_fwd<KS, 4, 4, 1, 1>(c);
    case 3: return launch_fwd<KS, 16, 4, 1, 2>(c);
    case 4: return launch_fwd<KS, 8, 4, 1, 2>(c);
    case 5: return launch_fwd<KS, 4, 4, 1, 2>(c);
    case 6: return launch_fwd<KS, 8, 2, 2, 4>(c);
    case 7: return launch_fwd<KS, 4, 1, 4, 4>(c);
    case 8: return launch_fwd<KS, 8, 4, 1, 4>(c);
    case 9: return launch_fwd<KS, 4, 2, 2, 4>(c);
    case 10: return launch_fwd<KS, 8, 2, 2, 2>(c);
    case 11: return launch_fwd<KS, 16, 2, 2, 2>(c);
    default: break;
  }
  if (KS == 3) {
    switch (cfg) {
      case 20: return launch_fwd_p<3, 8, 1, 1>(c);
      case 21: return launch_fwd_p<3, 8, 1, 2>(c);
      case 22: return launch_fwd_p<3, 16, 1, 1>(c);
      case 23: return launch_fwd_p<3, 16, 1, 2>(c);
      case 24: return launch_fwd_p<3, 8, 2, 1>(c);
      case 25: return launch_fwd_p<3, 8, 2, 2>(c);
      case 26: return launch_fwd_p<3, 16, 2, 1>(c);
      case 27: return launch_fwd_p<3, 16, 2, 2>(c);
      case 28: return launch_fwd_p<3, 8, 1, 4>(c);
      case 29: return launch_fwd_p<3, 16, 1, 4>(c);
      case 30: return launch_fwd_p<3, 16, 1, 1, false, false, true>(c);      // Winograd F(2x2,3x3) forms
      case 31: return launch_fwd_p<3, 16, 1, 2, false, false, true>(c);
      case 32: return launch_fwd_p<3, 16, 1, 4, false, false, true>(c);
      default: break;
    }
  }
  return -1;
}

// ---- 4x4 stride-1 pad-1 convolutions on the matrix cores (networks.NLayerDiscriminator / PatchDiscriminator, reference
// network/networks.py:977-1032: 64 -> 128 -> 256 -> 512 channels -- the place where north_star's "4x4 conv inner contractions"
// live).  An even kernel has an asymmetric halo and an output one pixel smaller than its input, so these are separate kernels
// with explicit input / output extents instead of more parameters on the "same"-conv kernels above:
//   forward   x [N,Hi,Wi,K] -> y [N,Ho,Wo,Nd], Ho = Hi + 2*pad - 3, pad = 1
//   dgrad     the same kernel on gy [N,Hi-1,Wi-1,Cout] with pad = 2, weights read transposed and tap-flipped -> gx [N,Hi,Wi,Cin]
// Same tiling as conv_mfma_fwd: TH x 16 output pixels x 16*NTN channels per workgroup, 16-channel K chunks staged in LDS with
// the halo ((TH+3) x 19 pixels, stride 24 floats), 16 taps x 4 MFMAs per chunk and accumulator tile, next chunk prefetched
// into registers under the MFMAs.
template <int TH, int NTN>
__global__ void __launch_bounds__(TPB)
conv_k4_fwd(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, int Hi, int Wi, int Ho, int Wo,
            int Kdim, int Ndim, int tiles_x, int pad, int transposed) {
  constexpr int KS = 4, KK = 16;
  constexpr int IH = TH + KS - 1, IW = TW + KS - 1;
  constexpr int CO_T = 16 * NTN, MR = TH / 4, NR = NTN;
  extern __shared__ float smem[];
  float* in_s = smem;                        // [IH][IW][SPIX]
  float* w_s = smem + IH * IW * SPIX;        // [KK][4][CO_T][4]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lm = lane & 15, kq = lane >> 4;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x % tiles_x;
  const int n_img = blockIdx.y, co0 = blockIdx.z * CO_T;
  const int y0 = ty * TH, x0 = tx * TW;
  const float* xin = x + (size_t)n_img * Hi * Wi * Kdim;
  f32x4 acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  constexpr int NI = (IH * IW * 4 + TPB - 1) / TPB, NW = (KK * 4 * CO_T + TPB - 1) / TPB;
  float4 rin[NI], rw[NW];
  int in_off[NI], w_off[NW];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int u = tid + i * TPB, q = u & 3, pix = u >> 2;
    const int gy_ = y0 + pix / IW - pad, gx_ = x0 + pix % IW - pad;
    in_off[i] = (u < IH * IW * 4 && gy_ >= 0 && gy_ < Hi && gx_ >= 0 && gx_ < Wi) ? (gy_ * Wi + gx_) * Kdim + 4 * q : -1;
  }
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int u = tid + i * TPB, n = u % CO_T, k4 = (u / CO_T) & 3, tap = u / (4 * CO_T), ng = co0 + n;
    w_off[i] = !(u < KK * 4 * CO_T && ng < Ndim) ? -1
               : (!transposed ? (tap * Kdim + 4 * k4) * Ndim + ng : ((KK - 1 - tap) * Ndim + ng) * Kdim + 4 * k4);
  }
  auto prefetch = [&](int c0) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in_off[i] >= 0 && c0 + 4 * ((tid + i * TPB) & 3) < Kdim) v = *(const float4*)(xin + in_off[i] + c0);
      rin[i] = v;
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int k4 = ((tid + i * TPB) / CO_T) & 3;
      if (w_off[i] >= 0 && c0 + 4 * k4 < Kdim) {
        if (!transposed) {
          const float* p = w + w_off[i] + (size_t)c0 * Ndim;
          v.x = p[0]; v.y = p[Ndim]; v.z = p[2 * (size_t)Ndim]; v.w = p[3 * (size_t)Ndim];
        } else v = *(const float4*)(w + w_off[i] + c0);
      }
      rw[i] = v;
    }
  };
  prefetch(0);
  for (int c0 = 0; c0 < Kdim; c0 += CK) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int u = tid + i * TPB;
      if (u < IH * IW * 4) *(float4*)(in_s + (u >> 2) * SPIX + 4 * (u & 3)) = rin[i];
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const int u = tid + i * TPB;
      if (u < KK * 4 * CO_T) *(float4*)(w_s + (size_t)u * 4) = rw[i];
    }
    __syncthreads();
    if (c0 + CK < Kdim) prefetch(c0 + CK);
#pragma unroll
    for (int tap = 0; tap < KK; ++tap) {
      const int kh = tap / KS, kw = tap % KS;
      f32x4 a[MR], b[NR];
#pragma unroll
      for (int i = 0; i < MR; ++i) a[i] = *(const f32x4*)(in_s + ((wave * MR + i + kh) * IW + lm + kw) * SPIX + 4 * kq);
#pragma unroll
      for (int j = 0; j < NR; ++j) b[j] = *(const f32x4*)(w_s + (((tap * 4 + kq) * CO_T) + j * 16 + lm) * 4);
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
        for (int i = 0; i < MR; ++i)
#pragma unroll
          for (int j = 0; j < NR; ++j) acc[i][j] = mfma16(a[i][s4], b[j][s4], acc[i][j]);
    }
  }
  float* yout = y + (size_t)n_img * Ho * Wo * Ndim;
#pragma unroll
  for (int i = 0; i < MR; ++i) {
    const int gy_ = y0 + wave * MR + i;
    if (gy_ >= Ho) continue;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const int co = co0 + j * 16 + lm;
      if (co >= Ndim) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gx_ = x0 + 4 * kq + r;
        if (gx_ < Wo) yout[((size_t)gy_ * Wo + gx_) * Ndim + co] = acc[i][j][r];
      }
    }
  }
}

// ---- what every conv entry point below shares ------------------------------------------------------------------------------------
// the operands, shape and stream of a call; the entry point then sets its few other fields by name
inline ConvCall conv_call(const void* x, const float* w, void* y, int N, int H, int W, int Kdim, int Ndim, void* stream) {
  ConvCall c;
  c.x = x; c.w = w; c.y = y;
  c.N = N; c.H = H; c.W = W; c.Kdim = Kdim; c.Ndim = Ndim;
  c.stream = (hipStream_t)stream;
  return c;
}
// the C ABI's `transposed` bit set, decoded once: bit 0 = transposed weights (data-gradient), bit 1 = accumulate into y
inline void set_transposed(ConvCall& c, int transposed) {
  c.transposed_w = (transposed & 1) != 0;
  c.accumulate = (transposed & 2) != 0;
}
inline int finish(int rc) {                   // rc of a launcher: -1 = the form is not covered, nothing launched
  SMSUT_REQUIRE(rc == 0);
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}
inline int run_p(const ConvCall& c) { return finish(select_fwd_p(c)); }       // persistent / Winograd kernels only
inline int run(const ConvCall& c, int KS = 3) { return finish(KS == 1 ? dispatch_fwd<1>(c) : dispatch_fwd<3>(c)); }

}  // namespace

extern "C" {

#ifdef SMSUT_STAMPS
int smsut_dbg_set_stamps(void* buf, int base) {
  hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_base), &base, sizeof(base));
  return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &buf, sizeof(buf));
}
#endif

// 1 when the MFMA kernels cover conv(k=KS, stride 1, pad (KS-1)/2) with this K (reduction) / N (output) channel pair
int smsut_conv2d_mfma_supported(int KS, int stride, int pad, int Kdim, int Ndim) {
  return (KS == 1 || KS == 3) && stride == 1 && pad == (KS - 1) / 2 && Kdim >= 4 && (Kdim % 4) == 0 && Ndim >= 1;
}

// Forward (transposed = 0): x [N,H,W,Kdim], w [KS*KS][Kdim][Ndim] -> y [N,H,W,Ndim].
// Data-gradient (transposed = 1): x = gy [N,H,W,Kdim = Cout], w = the forward weights [KS*KS][Ndim = Cin][Kdim = Cout],
// y = gx [N,H,W,Ndim = Cin].
// `_pre` forms (every 3x3 entry point that may run the streamed-weight Winograd kernel, conv_wino.hip): wu = the caller's prepared
// image of w for this form -- smsut_wino_prepare with the same (Kdim, Ndim) and the same bit 0 of `transposed` -- or NULL = the
// weights are transformed on the fly.  The image is only read when that kernel takes the shape; results are bit-identical either
// way.  The library keeps no table of images (r03 did): what is prepared, for how long it is valid and when it is passed is the
// caller's business (no process-wide mutable state behind the C ABI).
int smsut_conv2d_fwd_mfma_pre(const float* x, const float* w, float* y, int N, int H, int W, int Kdim, int Ndim, int KS,
                              int transposed, const float* wu, void* stream) {
  SMSUT_REQUIRE(x && w && y && N > 0 && H > 0 && W > 0);
  SMSUT_REQUIRE(smsut_conv2d_mfma_supported(KS, 1, (KS - 1) / 2, Kdim, Ndim));
  SMSUT_REQUIRE(!transposed || (Kdim % 4) == 0);
  ConvCall c = conv_call(x, w, y, N, H, W, Kdim, Ndim, stream);
  set_transposed(c, transposed);
  c.wu = wu;
  return run(c, KS);
}
int smsut_conv2d_fwd_mfma(const float* x, const float* w, float* y, int N, int H, int W, int Kdim, int Ndim, int KS,
                          int transposed, void* stream) {
  return smsut_conv2d_fwd_mfma_pre(x, w, y, N, H, W, Kdim, Ndim, KS, transposed, nullptr, stream);
}

// conv2 of a BasicBlock on the RAW conv1 output: y = conv3x3(lrelu(IN(x; mean, rstd, gamma, beta))) + statistics of y, the
// normalisation applied while the tiles are staged (a1 never exists in HBM).  Persistent-kernel shapes only
// (smsut_conv2d_mfma_persistent); statistics tiles as smsut_conv2d_mfma_tiles(N, H, W, Kdim, Ndim, 3).
int smsut_conv2d_fwd_mfma_stats_inaff_pre(const float* x, const float* w, float* y, float* stats, const float* mean,
                                          const float* rstd, const float* gamma, const float* beta, float slope, int N, int H,
                                          int W, int Kdim, int Ndim, const float* wu, void* stream) {
  SMSUT_REQUIRE(x && w && y && stats && mean && rstd && gamma && beta && N > 0 && H > 0 && W > 0);
  SMSUT_REQUIRE(fwd_any_eligible(N, H, W, Kdim, Ndim, false));
  const AffRef a{mean, rstd, gamma, beta, slope};
  ConvCall c = conv_call(x, w, y, N, H, W, Kdim, Ndim, stream);
  c.stats = stats; c.aff = &a; c.wu = wu;
  return run_p(c);
}
int smsut_conv2d_fwd_mfma_stats_inaff(const float* x, const float* w, float* y, float* stats, const float* mean,
                                      const float* rstd, const float* gamma, const float* beta, float slope, int N, int H,
                                      int W, int Kdim, int Ndim, void* stream) {
  return smsut_conv2d_fwd_mfma_stats_inaff_pre(x, w, y, stats, mean, rstd, gamma, beta, slope, N, H, W, Kdim, Ndim, nullptr, stream);
}

// conv1 of a BasicBlock fused with the block's 1x1 shortcut conv (network/blocks.py:66-80; both read the block input):
//   y = conv3x3(x, w), ysc = conv1x1(x, wsc), InstanceNorm partials of both (stats / stats_sc, tiles as
//   smsut_conv2d_mfma_tiles(N, H, W, Kdim, Ndim, 3)).  xb != null: x is the virtual cat([x, xb]) of two [N,H,W,Kdim/2] tensors.
// w [3][3][Kdim][Ndim], wsc [Kdim][Ndim] (HWIO).  Persistent-kernel shapes with Kdim in {16, 32, 64}: _supported says which.
int smsut_conv2d_fwd_sc_supported(int N, int H, int W, int Kdim, int Ndim, int cat) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  if (wino_l_shape(N, H, W, Kdim, Ndim)) return (!cat || Kdim % 32 == 0) ? 1 : 0;       // (conv_wino.hip: any reduction width)
  if (!(Kdim == 8 || Kdim == 16 || Kdim == 32 || Kdim == 64) || !fwd_p_eligible(N, H, W, Kdim, Ndim)) return 0;
  if (cat && Kdim % 32 != 0) return 0;
  return 1;
}

int smsut_conv2d_fwd_mfma_stats_sc_pre(const float* x, const float* xb, const float* w, const float* wsc, float* y, float* ysc,
                                       float* stats, float* stats_sc, int N, int H, int W, int Kdim, int Ndim, const float* wu,
                                       void* stream) {
  SMSUT_REQUIRE(x && w && wsc && y && ysc && stats && stats_sc && smsut_conv2d_fwd_sc_supported(N, H, W, Kdim, Ndim, xb != nullptr));
  const ScRef sc{wsc, ysc, stats_sc};
  ConvCall c = conv_call(x, w, y, N, H, W, Kdim, Ndim, stream);
  c.x2 = xb; c.stats = stats; c.sc = &sc; c.wu = wu;
  return run_p(c);
}
int smsut_conv2d_fwd_mfma_stats_sc(const float* x, const float* xb, const float* w, const float* wsc, float* y, float* ysc,
                                   float* stats, float* stats_sc, int N, int H, int W, int Kdim, int Ndim, void* stream) {
  return smsut_conv2d_fwd_mfma_stats_sc_pre(x, xb, w, wsc, y, ysc, stats, stats_sc, N, H, W, Kdim, Ndim, nullptr, stream);
}
// ... with fp16 operands (BASELINE config 5): the persistent kernel's direct form, Kdim in {16, 32, 64} (the fp16-operand mode has
// no Winograd forms); statistics tiles = smsut_conv2d_mfma_tiles(N, H, W, Kdim, Ndim, 3, /*f16=*/1).
int smsut_conv2d_fwd_sc_f16_supported(int N, int H, int W, int Kdim, int Ndim, int cat) {
  if (N <= 0 || H <= 0 || W <= 0 || !(Kdim == 16 || Kdim == 32 || Kdim == 64) || !fwd_p_eligible(N, H, W, Kdim, Ndim)) return 0;
  if (cat && Kdim % 32 != 0) return 0;
  return 1;
}
int smsut_conv2d_fwd_mfma_stats_sc_f16(const float* x, const float* xb, const float* w, const float* wsc, float* y, float* ysc,
                                       float* stats, float* stats_sc, int N, int H, int W, int Kdim, int Ndim, void* stream) {
  SMSUT_REQUIRE(x && w && wsc && y && ysc && stats && stats_sc && smsut_conv2d_fwd_sc_f16_supported(N, H, W, Kdim, Ndim, xb != nullptr));
  const ScRef sc{wsc, ysc, stats_sc};
  ConvCall c = conv_call(x, w, y, N, H, W, Kdim, Ndim, stream);
  c.x2 = xb; c.stats = stats; c.sc = &sc; c.f16_operands = true;
  return run_p(c);
}

// Data-gradient of that pair: gx = dgrad3x3(gy, w) + dgrad1x1(gs, wsc) in one pass (gy, gs [N,H,W,Cout]; w, wsc the forward
// weights [3][3][Cin][Cout], [Cin][Cout]).  gxb != null: channels [0, split) of gx go to gxa [N,H,W,split], the rest to gxb
// (block input was cat([up, skip])).  Persistent-kernel shapes with Cout in {16, 32}: _supported says which.
int smsut_conv2d_dgrad_sc_supported(int N, int H, int W, int Cout, int Cin, int split) {
  if (N <= 0 || H <= 0 || W <= 0 || !(Cout == 16 || Cout == 32)) return 0;
  if (Cin == 8) return !split && Cout == 16 && fwd_p_n8_eligible(N, H, W, 2 * Cout, Cin);       // first block after the stem: 8-channel result
  if (!fwd_any_eligible(N, H, W, 2 * Cout, Cin, false)) return 0;
  if (split && (split <= 0 || split >= Cin || split % 16 != 0 || (Cin - split) % 16 != 0)) return 0;
  return 1;
}

int smsut_conv2d_dgrad_mfma_sc(const float* gy, const float* gs, const float* w, const float* wsc, float* gxa, float* gxb,
                               int split, int N, int H, int W, int Cout, int Cin, void* stream) {
  SMSUT_REQUIRE(gy && gs && w && wsc && gxa && smsut_conv2d_dgrad_sc_supported(N, H, W, Cout, Cin, gxb ? split : 0));
  const ScRef sc{wsc, nullptr, nullptr};
  ConvCall c = conv_call(gy, w, gxa, N, H, W, 2 * Cout, Cin, stream);
  c.x2 = gs; c.y2 = gxb; c.split = gxb ? split : 0; c.sc = &sc; c.transposed_w = true;
  return run_p(c);
}

// fp16 RESULT STORAGE (config 5, r04): the same passes, the raw conv outputs y (and ysc) stored as fp16 [N,H,W,Ndim] -- block-internal
// tensors of a BasicBlock (its consumers: smsut_restail_*_hs).  Persistent-kernel shapes, Kdim in {16, 32, 64}; xb nullable
// (virtual cat); InstanceNorm partials as in the fp32-storage forms (tiles with f16 = 1).
// Kdim == 8 (the first block after the stem): the fused-shortcut form only, fp32 operands (no fp16 twin), same fp16 storage.
int smsut_conv2d_f16_hs_supported(int N, int H, int W, int Kdim, int Ndim, int cat) {
  if (N <= 0 || H <= 0 || W <= 0 || !fwd_p_eligible(N, H, W, Kdim, Ndim)) return 0;
  if (Kdim == 8) return !cat && smsut_conv2d_fwd_sc_supported(N, H, W, Kdim, Ndim, 0);
  if (!(Kdim == 16 || Kdim == 32 || Kdim == 64)) return 0;
  return !(cat && Kdim % 32 != 0);
}
int smsut_conv2d_fwd_mfma_stats_f16_hs(const float* x, const float* xb, const float* w, void* y16, float* stats, int N, int H, int W,
                                       int Kdim, int Ndim, void* stream) {
  SMSUT_REQUIRE(x && w && y16 && stats && Kdim != 8 && smsut_conv2d_f16_hs_supported(N, H, W, Kdim, Ndim, xb != nullptr));
  ConvCall c = conv_call(x, w, y16, N, H, W, Kdim, Ndim, stream);
  c.x2 = xb; c.stats = stats; c.f16_operands = true; c.out_f16 = true;
  return run_p(c);
}
// ... whose INPUT is fp16 as well (conv2 of the block reading the activated a1 that smsut_instnorm_fwd_partials_hs2 stored as fp16):
// the operands are the bits the fp32-input form rounds a1 to -- same result, 2 bytes per element less to read
int smsut_conv2d_fwd_mfma_stats_f16_hsx(const void* x16, const float* w, void* y16, float* stats, int N, int H, int W, int Kdim,
                                        int Ndim, void* stream) {
  SMSUT_REQUIRE(x16 && w && y16 && stats && smsut_conv2d_f16_hs_supported(N, H, W, Kdim, Ndim, 0));
  ConvCall c = conv_call(x16, w, y16, N, H, W, Kdim, Ndim, stream);
  c.stats = stats; c.f16_operands = true; c.in_f16 = true; c.out_f16 = true;
  return run_p(c);
}
// ... reading the RAW fp16 conv1 output y1 and applying lrelu(IN(.)) while staging (mean / rstd [N,Kdim], gamma / beta [Kdim]): the
// half-storage twin of smsut_conv2d_fwd_mfma_stats_inaff -- the activated a1 is never built
int smsut_conv2d_fwd_mfma_stats_inaff_f16_hsx(const void* y1_16, const float* w, void* y16, float* stats, const float* mean,
                                              const float* rstd, const float* gamma, const float* beta, float slope, int N, int H,
                                              int W, int Kdim, int Ndim, void* stream) {
  SMSUT_REQUIRE(y1_16 && w && y16 && stats && mean && rstd && gamma && beta && Kdim != 8 && smsut_conv2d_f16_hs_supported(N, H, W, Kdim, Ndim, 0));
  const AffRef a{mean, rstd, gamma, beta, slope};
  ConvCall c = conv_call(y1_16, w, y16, N, H, W, Kdim, Ndim, stream);
  c.stats = stats; c.aff = &a; c.f16_operands = true; c.in_f16 = true; c.out_f16 = true;
  return run_p(c);
}
int smsut_conv2d_fwd_mfma_stats_sc_f16_hs(const float* x, const float* xb, const float* w, const float* wsc, void* y16, void* ysc16,
                                          float* stats, float* stats_sc, int N, int H, int W, int Kdim, int Ndim, void* stream) {
  SMSUT_REQUIRE(x && w && wsc && y16 && ysc16 && stats && stats_sc && smsut_conv2d_f16_hs_supported(N, H, W, Kdim, Ndim, xb != nullptr) &&
                (Kdim == 8 || smsut_conv2d_fwd_sc_f16_supported(N, H, W, Kdim, Ndim, xb != nullptr)));
  const ScRef sc{wsc, (float*)ysc16, stats_sc};      // (the kernel argument's type; fp16 storage under out_f16)
  ConvCall c = conv_call(x, w, y16, N, H, W, Kdim, Ndim, stream);
  c.x2 = xb; c.stats = stats; c.sc = &sc; c.f16_operands = Kdim != 8; c.out_f16 = true;
  return run_p(c);
}

// conv2's data-gradient with the IN1 / LeakyReLU mask and backward statistics (smsut_conv2d_dgrad_mfma_bwdstats_f16) reading an fp16 y1
int smsut_conv2d_dgrad_mfma_bwdstats_f16_hs(const float* gy, const float* w, float* gz, float* stats, const void* y1_16,
                                            const float* mean, const float* rstd, const float* gamma, const float* beta,
                                            const float* gsc, float slope, int N, int H, int W, int Kdim, int Ndim, void* stream) {
  SMSUT_REQUIRE(gy && w && gz && stats && y1_16 && mean && rstd && gamma && beta && smsut_conv2d_f16_hs_supported(N, H, W, Kdim, Ndim, 0));
  const BstRef b{(const float*)y1_16, mean, rstd, gamma, beta, slope};      // (the kernel argument's type; fp16 storage under out_f16)
  ConvCall c = conv_call(gy, w, gz, N, H, W, Kdim, Ndim, stream);
  c.stats = stats; c.bst = &b; c.gsc = gsc; c.transposed_w = true; c.f16_operands = true; c.out_f16 = true;
  return run_p(c);
}

// ... with fp16 operands (config 5): gsc = {s, 1/s} of smsut_absmax_scale2(gy, gs) -- the two gradients share the accumulators, so
// they share the scale.  Direct resident-weight form (16 / 32 -> Cin >= 16).
int smsut_conv2d_dgrad_sc_f16_supported(int N, int H, int W, int Cout, int Cin, int split) {
  if (N <= 0 || H <= 0 || W <= 0 || !(Cout == 16 || Cout == 32) || Cin < 16 || !fwd_p_eligible(N, H, W, 2 * Cout, Cin)) return 0;
  if (split && (split <= 0 || split >= Cin || split % 16 != 0 || (Cin - split) % 16 != 0)) return 0;
  return 1;
}
int smsut_conv2d_dgrad_mfma_sc_f16(const float* gy, const float* gs, const float* w, const float* wsc, float* gxa, float* gxb,
                                   const float* gsc, int split, int N, int H, int W, int Cout, int Cin, void* stream) {
  SMSUT_REQUIRE(gy && gs && w && wsc && gxa && gsc && smsut_conv2d_dgrad_sc_f16_supported(N, H, W, Cout, Cin, gxb ? split : 0));
  const ScRef sc{wsc, nullptr, nullptr};
  ConvCall c = conv_call(gy, w, gxa, N, H, W, 2 * Cout, Cin, stream);
  c.x2 = gs; c.y2 = gxb; c.split = gxb ? split : 0; c.sc = &sc; c.gsc = gsc; c.transposed_w = true; c.f16_operands = true;
  return run_p(c);
}

// Which arithmetic a 3x3 stride-1 fp32 conv call (forward or data-gradient, any fused form) runs for this shape: 0 = direct
// products (36 per 2x2 output tile and channel pair), 1 = Winograd F(2x2,3x3) with resident weights (conv_mfma_fwd_p<..,WINO>),
// 2 = Winograd with streamed weights (conv_wino_l) -- 16 products per tile.  Mirrors select_fwd_p / dispatch_fwd; sc_dgrad = the
// fused shortcut data-gradient (Kdim = 2 Cout).  bench.py / profiling.py use it to report the FLOPs the matrix pipes EXECUTE.
int smsut_conv2d_mfma_form(int N, int H, int W, int Kdim, int Ndim, int sc_dgrad) {
  if (N <= 0 || H <= 0 || W <= 0 || !fwd_any_eligible(N, H, W, Kdim, Ndim, false)) return 0;
  const bool sc2_64 = sc_dgrad && Kdim == 64 && fwd_p_eligible(N, H, W, Kdim, Ndim);
  if (!sc2_64 && wino_l_shape(N, H, W, Kdim, Ndim)) return 2;
  if (Ndim == 8 || Kdim == 8) return 0;
  return (winograd_on() && H % 16 == 0 && (Kdim == 16 || Kdim == 32) && fwd_p_eligible(N, H, W, Kdim, Ndim)) ? 1 : 0;
}


// Forward 3x3 conv + InstanceNorm partials (as smsut_conv2d_fwd_mfma_stats) of the virtual cat([xa, xb]) of two
// [N,H,W,Kdim/2] tensors, read in place.  Persistent kernel, Kdim in {32, 64}: _supported says whether the shape is covered;
// the statistics tiles are those of smsut_conv2d_mfma_tiles(N, H, W, Kdim, Ndim, 3).
int smsut_conv2d_mfma_cat_supported(int N, int H, int W, int Kdim, int Ndim) {
  // persistent kernel (Kdim 32 / 64) or the per-tile kernel: two halves of whole 16-channel chunks
  return N > 0 && H > 0 && W > 0 && Kdim % 32 == 0 && smsut_conv2d_mfma_supported(3, 1, 1, Kdim, Ndim) &&
         (int64_t)N * H * W * (Kdim > Ndim ? Kdim : Ndim) < (1ll << 31);
}

int smsut_conv2d_fwd_mfma_stats_cat_pre(const float* xa, const float* xb, const float* w, float* y, float* stats, int N, int H,
                                        int W, int Kdim, int Ndim, const float* wu, void* stream) {
  SMSUT_REQUIRE(xa && xb && w && y && stats && smsut_conv2d_mfma_cat_supported(N, H, W, Kdim, Ndim));
  ConvCall c = conv_call(xa, w, y, N, H, W, Kdim, Ndim, stream);
  c.x2 = xb; c.stats = stats; c.wu = wu;
  return run(c);
}
int smsut_conv2d_fwd_mfma_stats_cat(const float* xa, const float* xb, const float* w, float* y, float* stats, int N, int H,
                                    int W, int Kdim, int Ndim, void* stream) {
  return smsut_conv2d_fwd_mfma_stats_cat_pre(xa, xb, w, y, stats, N, H, W, Kdim, Ndim, nullptr, stream);
}

// 3x3 conv (any `transposed` form of smsut_conv2d_fwd_mfma) whose result channels [0, split) go to ya [N,H,W,split] and
// [split, Ndim) to yb [N,H,W,Ndim-split]: the data-gradient of a block fed by cat([up, skip]) (network/blocks.py:49)
// written straight into the two gradients.  Persistent kernel only: _supported tells whether this shape is covered.
int smsut_conv2d_mfma_split_supported(int N, int H, int W, int Kdim, int Ndim, int split) {
  // 16-channel output tiles never straddle the seam
  if (N <= 0 || H <= 0 || W <= 0 || split <= 0 || split >= Ndim || split % 16 != 0 ||
      !smsut_conv2d_mfma_supported(3, 1, 1, Kdim, Ndim) || Kdim % 4 != 0)
    return 0;
  return 1;          // a persistent variant that cannot split at `split` declines and the per-tile kernel takes over
}

int smsut_conv2d_fwd_mfma_split_pre(const float* x, const float* w, float* ya, float* yb, int split, int N, int H, int W,
                                    int Kdim, int Ndim, int transposed, const float* wu, void* stream) {
  SMSUT_REQUIRE(x && w && ya && yb && N > 0 && H > 0 && W > 0 && (transposed & ~3) == 0);
  SMSUT_REQUIRE(smsut_conv2d_mfma_split_supported(N, H, W, Kdim, Ndim, split));
  ConvCall c = conv_call(x, w, ya, N, H, W, Kdim, Ndim, stream);
  set_transposed(c, transposed);
  c.y2 = yb; c.split = split; c.wu = wu;
  return run(c);
}
int smsut_conv2d_fwd_mfma_split(const float* x, const float* w, float* ya, float* yb, int split, int N, int H, int W,
                                int Kdim, int Ndim, int transposed, void* stream) {
  return smsut_conv2d_fwd_mfma_split_pre(x, w, ya, yb, split, N, H, W, Kdim, Ndim, transposed, nullptr, stream);
}

// ConvTranspose2d(k=2, s=2, bias=False) (network/blocks.py:41), weights [kh][kw][Cin][Cout]:
//   forward  x [N,H,W,Cin] -> y [N,2H,2W,Cout]   : four 1x1 MFMA convs scattered to the 4 output taps
//   dgrad    gy [N,2H,2W,Cout] -> gx [N,H,W,Cin] : one 1x1 MFMA conv over the 4 gathered taps (K = 4*Cout)
//   wgrad    gw[tap] = sum_p x[p] (x) gy[2p + tap]          (smsut_convT2x2_wgrad_mfma, conv_mfma_wgrad.hip)
int smsut_convT2x2_mfma_supported(int Cin, int Cout) { return Cin >= 4 && (Cin % 4) == 0 && Cout >= 4 && (Cout % 4) == 0; }

int smsut_convT2x2_fwd_mfma(const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout,
                            void* stream) {
  SMSUT_REQUIRE(x && w && y && N > 0 && H > 0 && W > 0 && smsut_convT2x2_mfma_supported(Cin, Cout));
  ConvCall c = conv_call(x, w, y, N, H, W, Cin, Cout, stream);
  c.osc = 2; c.ntap_out = 4;
  return run(c, 1);
}

int smsut_convT2x2_dgrad_mfma(const float* gy, const float* w, float* gx, int N, int H, int W, int Cin, int Cout,
                              void* stream) {
  SMSUT_REQUIRE(gy && w && gx && N > 0 && H > 0 && W > 0 && smsut_convT2x2_mfma_supported(Cin, Cout));
  ConvCall c = conv_call(gy, w, gx, N, H, W, Cout, Cin, stream);
  c.transposed_w = true; c.isc = 2; c.G = 4;
  return run(c, 1);
}

// Forward conv that also emits the InstanceNorm statistics partials of its output (see conv_mfma_fwd).
// stats: float[N * smsut_conv2d_mfma_tiles(N, H, W, Kdim, Ndim, KS) * Ndim * 2]
// (the kernel variant and its tile shape depend on the whole layer shape, so all of it is part of the query)
int smsut_conv2d_mfma_tiles(int N, int H, int W, int Kdim, int Ndim, int KS, int f16) {
  // f16: the tiles of the fp16-operand entry points (r03: the fp32 forms of a shape may run a Winograd kernel on 16-row items
  // where the fp16 ones keep the direct kernel's)
  int tiles = 0;
  ConvCall c = conv_call(nullptr, nullptr, nullptr, N, H, W, Kdim, Ndim, nullptr);
  c.tiles_out = &tiles;
  c.f16_operands = KS != 1 && f16 != 0;
  if (KS == 1) dispatch_fwd<1>(c);
  else dispatch_fwd<3>(c);
  return tiles;
}

// 1 when conv(k=KS) on this shape runs the persistent resident-weight kernel (conv_mfma_fwd_p), 0 for the per-tile kernel
int smsut_conv2d_mfma_persistent(int N, int H, int W, int Kdim, int Ndim, int KS, int f16) {
  return KS == 3 && fwd_any_eligible(N, H, W, Kdim, Ndim, f16 != 0) ? 1 : 0;
}

int smsut_conv2d_fwd_mfma_stats_pre(const float* x, const float* w, float* y, float* stats, int N, int H, int W, int Kdim,
                                    int Ndim, int KS, const float* wu, void* stream) {
  SMSUT_REQUIRE(x && w && y && stats && N > 0 && H > 0 && W > 0);
  SMSUT_REQUIRE(smsut_conv2d_mfma_supported(KS, 1, (KS - 1) / 2, Kdim, Ndim));
  ConvCall c = conv_call(x, w, y, N, H, W, Kdim, Ndim, stream);
  c.stats = stats;
  c.wu = wu;
  return run(c, KS);
}
int smsut_conv2d_fwd_mfma_stats(const float* x, const float* w, float* y, float* stats, int N, int H, int W, int Kdim,
                                int Ndim, int KS, void* stream) {
  return smsut_conv2d_fwd_mfma_stats_pre(x, w, y, stats, N, H, W, Kdim, Ndim, KS, nullptr, stream);
}

// Data-gradient of a 3x3 conv whose input was a = LeakyReLU(IN(y1)) (conv2 of a BasicBlock): writes gz = g * mask(y1) and the
// per-tile partials {sum gz, sum gz * xhat} [N][tiles][Ndim][2] of the InstanceNorm backward (tiles =
// smsut_conv2d_mfma_tiles(N, H, W, Kdim, Ndim, 3)).  Only where smsut_conv2d_mfma_persistent(...) == 1; -1 otherwise.
int smsut_conv2d_dgrad_mfma_bwdstats_pre(const float* gy, const float* w, float* gz, float* stats, const float* y1,
                                         const float* mean, const float* rstd, const float* gamma, const float* beta,
                                         float slope, int N, int H, int W, int Kdim, int Ndim, const float* wu, void* stream) {
  SMSUT_REQUIRE(gy && w && gz && stats && y1 && mean && rstd && gamma && beta && N > 0 && H > 0 && W > 0);
  SMSUT_REQUIRE(fwd_any_eligible(N, H, W, Kdim, Ndim, false));
  const BstRef b{y1, mean, rstd, gamma, beta, slope};
  ConvCall c = conv_call(gy, w, gz, N, H, W, Kdim, Ndim, stream);
  c.stats = stats; c.bst = &b; c.transposed_w = true; c.wu = wu;
  return run_p(c);
}
int smsut_conv2d_dgrad_mfma_bwdstats(const float* gy, const float* w, float* gz, float* stats, const float* y1,
                                     const float* mean, const float* rstd, const float* gamma, const float* beta,
                                     float slope, int N, int H, int W, int Kdim, int Ndim, void* stream) {
  return smsut_conv2d_dgrad_mfma_bwdstats_pre(gy, w, gz, stats, y1, mean, rstd, gamma, beta, slope, N, H, W, Kdim, Ndim, nullptr, stream);
}

// ---- `_fin` forms (r05): the same launches with the InstanceNorm statistics FINALISED INSIDE THE LAUNCH (common.h, FinRef): the
// workgroup whose partials complete an image combines them (in_moments_final's order: same bits) -- the separate
// smsut_in_finalize_* launch behind every statistics-producing conv of a fused BasicBlock (network/blocks.py:70-79 of the original model:
// conv -> InstanceNorm, three times per block forward, once more per block backward) disappears.  tickets: int [N], ZERO on entry,
// zero again when the launch is over (the caller hands out slices of one zero-initialised pool).  wu (nullable): the caller's
// prepared Winograd image for this call (the `_pre` argument).  fp32 operands.
int smsut_conv2d_fwd_mfma_stats_sc_fin(const float* x, const float* xb, const float* w, const float* wsc, float* y, float* ysc,
                                       float* stats, float* stats_sc, int* tickets, float* mean, float* rstd, float* mean_sc,
                                       float* rstd_sc, float eps, int N, int H, int W, int Kdim, int Ndim, const float* wu,
                                       void* stream) {
  SMSUT_REQUIRE(x && w && wsc && y && ysc && stats && stats_sc && tickets && mean && rstd && mean_sc && rstd_sc);
  SMSUT_REQUIRE(smsut_conv2d_fwd_sc_supported(N, H, W, Kdim, Ndim, xb != nullptr));
  const ScRef sc{wsc, ysc, stats_sc};
  const FinRef fin{tickets, mean, rstd, mean_sc, rstd_sc, eps};
  ConvCall c = conv_call(x, w, y, N, H, W, Kdim, Ndim, stream);
  c.x2 = xb; c.stats = stats; c.sc = &sc; c.fin = &fin; c.wu = wu;
  return run_p(c);
}
int smsut_conv2d_fwd_mfma_stats_inaff_fin(const float* x, const float* w, float* y, float* stats, const float* mean,
                                          const float* rstd, const float* gamma, const float* beta, float slope, int* tickets,
                                          float* mean_out, float* rstd_out, float eps, int N, int H, int W, int Kdim, int Ndim,
                                          const float* wu, void* stream) {
  SMSUT_REQUIRE(x && w && y && stats && mean && rstd && gamma && beta && tickets && mean_out && rstd_out && N > 0 && H > 0 && W > 0);
  SMSUT_REQUIRE(fwd_any_eligible(N, H, W, Kdim, Ndim, false));
  const AffRef a{mean, rstd, gamma, beta, slope};
  const FinRef fin{tickets, mean_out, rstd_out, nullptr, nullptr, eps};
  ConvCall c = conv_call(x, w, y, N, H, W, Kdim, Ndim, stream);
  c.stats = stats; c.aff = &a; c.fin = &fin; c.wu = wu;
  return run_p(c);
}
// ... the data-gradient with backward statistics: a_mean / b_mean [N][Ndim] = mean(gz), mean(gz * xhat) (what smsut_in_finalize_bwd writes)
int smsut_conv2d_dgrad_mfma_bwdstats_fin(const float* gy, const float* w, float* gz, float* stats, const float* y1,
                                         const float* mean, const float* rstd, const float* gamma, const float* beta, float slope,
                                         int* tickets, float* a_mean, float* b_mean, int N, int H, int W, int Kdim, int Ndim,
                                         const float* wu, void* stream) {
  SMSUT_REQUIRE(gy && w && gz && stats && y1 && mean && rstd && gamma && beta && tickets && a_mean && b_mean && N > 0 && H > 0 && W > 0);
  SMSUT_REQUIRE(fwd_any_eligible(N, H, W, Kdim, Ndim, false));
  const BstRef b{y1, mean, rstd, gamma, beta, slope};
  const FinRef fin{tickets, a_mean, b_mean, nullptr, nullptr, 0.f};
  ConvCall c = conv_call(gy, w, gz, N, H, W, Kdim, Ndim, stream);
  c.stats = stats; c.bst = &b; c.fin = &fin; c.transposed_w = true; c.wu = wu;
  return run_p(c);
}

int smsut_conv2d_fwd_mfma_cfg(const float* x, const float* w, float* y, int N, int H, int W, int Kdim, int Ndim, int KS,
                              int transposed, int cfg, void* stream) {
  SMSUT_REQUIRE(x && w && y && N > 0 && H > 0 && W > 0 && smsut_conv2d_mfma_supported(KS, 1, (KS - 1) / 2, Kdim, Ndim));
  ConvCall c = conv_call(x, w, y, N, H, W, Kdim, Ndim, stream);
  set_transposed(c, transposed);
  return finish(KS == 1 ? dispatch_fwd_cfg<1>(cfg, c) : dispatch_fwd_cfg<3>(cfg, c));
}

// ---- fp16-operand entry points (BASELINE config 5; see the block comment above mfma16h, conv_mfma.h) -----------------------------------
// Same tensors (fp32 in HBM), same tile selection and statistics layout as the fp32 entry points of the same name; operands
// are converted to fp16 while they are staged.  gsc (nullable): device float[2] = {s, 1/s} from smsut_absmax_scale for a
// GRADIENT input operand (x of a data-gradient form, gy of the weight gradient).
int smsut_conv2d_f16_supported(int KS, int Kdim, int Ndim) {
  return (KS == 1 || KS == 3) && Kdim >= 16 && Kdim % 16 == 0 && Ndim >= 1;
}
int smsut_conv2d_fwd_mfma_f16(const float* x, const float* w, float* y, const float* gsc, int N, int H, int W, int Kdim,
                              int Ndim, int KS, int transposed, void* stream) {
  SMSUT_REQUIRE(x && w && y && N > 0 && H > 0 && W > 0 && smsut_conv2d_f16_supported(KS, Kdim, Ndim));
  ConvCall c = conv_call(x, w, y, N, H, W, Kdim, Ndim, stream);
  set_transposed(c, transposed);
  c.gsc = gsc; c.f16_operands = true;
  return run(c, KS);
}
int smsut_conv2d_fwd_mfma_stats_f16(const float* x, const float* w, float* y, float* stats, int N, int H, int W, int Kdim,
                                    int Ndim, int KS, void* stream) {
  SMSUT_REQUIRE(x && w && y && stats && N > 0 && H > 0 && W > 0 && smsut_conv2d_f16_supported(KS, Kdim, Ndim));
  ConvCall c = conv_call(x, w, y, N, H, W, Kdim, Ndim, stream);
  c.stats = stats; c.f16_operands = true;
  return run(c, KS);
}
int smsut_conv2d_fwd_mfma_stats_cat_f16(const float* xa, const float* xb, const float* w, float* y, float* stats, int N,
                                        int H, int W, int Kdim, int Ndim, void* stream) {
  SMSUT_REQUIRE(xa && xb && w && y && stats && smsut_conv2d_mfma_cat_supported(N, H, W, Kdim, Ndim));
  ConvCall c = conv_call(xa, w, y, N, H, W, Kdim, Ndim, stream);
  c.x2 = xb; c.stats = stats; c.f16_operands = true;
  return run(c);
}
int smsut_conv2d_fwd_mfma_split_f16(const float* x, const float* w, float* ya, float* yb, const float* gsc, int split, int N,
                                    int H, int W, int Kdim, int Ndim, int transposed, void* stream) {
  SMSUT_REQUIRE(x && w && ya && yb && N > 0 && H > 0 && W > 0 && (transposed & ~3) == 0 && Kdim % 16 == 0);
  SMSUT_REQUIRE(smsut_conv2d_mfma_split_supported(N, H, W, Kdim, Ndim, split));
  ConvCall c = conv_call(x, w, ya, N, H, W, Kdim, Ndim, stream);
  set_transposed(c, transposed);
  c.y2 = yb; c.split = split; c.gsc = gsc; c.f16_operands = true;
  return run(c);
}
int smsut_conv2d_dgrad_mfma_bwdstats_f16(const float* gy, const float* w, float* gz, float* stats, const float* y1,
                                         const float* mean, const float* rstd, const float* gamma, const float* beta,
                                         const float* gsc, float slope, int N, int H, int W, int Kdim, int Ndim, void* stream) {
  SMSUT_REQUIRE(gy && w && gz && stats && y1 && mean && rstd && gamma && beta && N > 0 && H > 0 && W > 0);
  SMSUT_REQUIRE(fwd_p_eligible(N, H, W, Kdim, Ndim));
  const BstRef b{y1, mean, rstd, gamma, beta, slope};
  ConvCall c = conv_call(gy, w, gz, N, H, W, Kdim, Ndim, stream);
  c.stats = stats; c.bst = &b; c.gsc = gsc; c.transposed_w = true; c.f16_operands = true;
  return run_p(c);
}

// ---- 4x4 stride-1 pad-1 convolutions (networks.NLayerDiscriminator, reference network/networks.py:977-1032) -----------------
// (H, W) are always the extents of the conv's FORWARD INPUT; its output is (H-1) x (W-1).
int smsut_conv2d_k4_supported(int Cin, int Cout) { return Cin >= 4 && Cin % 4 == 0 && Cout >= 4 && Cout % 4 == 0; }
// transposed = 0: x [N,H,W,Cin] -> y [N,H-1,W-1,Cout];  transposed = 1: x = gy [N,H-1,W-1,Cout] -> y = gx [N,H,W,Cin]
int smsut_conv2d_k4_fwd(const float* x, const float* w, float* y, int N, int H, int W, int Cin, int Cout, int transposed,
                        void* stream) {
  SMSUT_REQUIRE(x && w && y && N > 0 && H > 1 && W > 1 && smsut_conv2d_k4_supported(Cin, Cout) && (transposed & ~1) == 0);
  SMSUT_REQUIRE((int64_t)N * H * W * (Cin > Cout ? Cin : Cout) < (1ll << 31));
  const int Hi = transposed ? H - 1 : H, Wi = transposed ? W - 1 : W, Ho = transposed ? H : H - 1, Wo = transposed ? W : W - 1;
  const int Kdim = transposed ? Cout : Cin, Ndim = transposed ? Cin : Cout, pad = transposed ? 2 : 1;
  constexpr int TH = 8;
  const int tiles_x = (Wo + TW - 1) / TW, tiles_y = (Ho + TH - 1) / TH;
  hipStream_t st = (hipStream_t)stream;
  if (Ndim % 32 == 0 || Ndim > 16) {
    constexpr size_t sh = (size_t)((TH + 3) * (TW + 3) * SPIX + 16 * CK * 32) * sizeof(float);
    conv_k4_fwd<TH, 2><<<dim3(tiles_x * tiles_y, N, (Ndim + 31) / 32), TPB, sh, st>>>(x, w, y, Hi, Wi, Ho, Wo, Kdim, Ndim, tiles_x,
                                                                                    pad, transposed);
  } else {
    constexpr size_t sh = (size_t)((TH + 3) * (TW + 3) * SPIX + 16 * CK * 16) * sizeof(float);
    conv_k4_fwd<TH, 1><<<dim3(tiles_x * tiles_y, N, (Ndim + 15) / 16), TPB, sh, st>>>(x, w, y, Hi, Wi, Ho, Wo, Kdim, Ndim, tiles_x,
                                                                                    pad, transposed);
  }
  SMSUT_LAUNCH_CHECK();
  return SMSUT_OK;
}

}  // extern "C"
