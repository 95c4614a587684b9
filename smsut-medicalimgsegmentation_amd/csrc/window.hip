// Sliding-window inference on the device (smsut_amd/predict.py: Predictor.predict_windows): the network runs at the window size it
// was trained on over overlapping windows of a larger slice, and the windows' class probabilities are blended on the slice's grid
// with a separable importance map (Gaussian or constant: ops.window_weights); the label and a confidence are taken from the blend.
//
// k_window_blend: ny * nx tiles of mean class probabilities, fp32 [N][wh][ww][K] each (what k_tta_merge writes as `prob`), tile
//   (iy, ix) lying at rows ys[iy] .. ys[iy] + wh - 1 and columns xs[ix] .. xs[ix] + ww - 1 of the grid [N][H][W]; each tile is read
//   in place through its own base pointer (a by-value table in the kernel arguments, nothing is stacked or copied) -> pred uint8
//   [N][H][W], optional conf fp32 [N][H][W], optional prob fp32 [N][H][W][K].
//   Per output pixel (n, y, x), all in fp32, the tiles that cover the pixel taken in row-major (iy, ix) order:
//     w_t = wy[y - ys[iy]] * wx[x - xs[ix]], rounded on its own;   s = w_0 + w_1 + ... in that order;   v_t = w_t / s (IEEE division);
//     acc_k = v_0 p_0[k] + v_1 p_1[k] + ... in that order from 0.0f (a product may be fused into its addition: one rounding less).
//   pred = the first maximum of acc_k by k_argmax_channels' comparison (the first maximum wins, a NaN wins), conf = acc_pred,
//   prob = acc.  The weights are normalised BEFORE the sum, so a pixel under one tile gets v = w / w = 1.0f exactly and its
//   probabilities pass through bit for bit.  A pixel that no tile covers (ops.window_blend refuses such a plan) gets acc = 0, pred 0.
//   A pixel belongs to one lane from its first load to its stores: no atomics, no cross-lane sums, so two calls are bitwise equal.
//
// Shape.  A gather: per pixel (covering tiles) * K * 4 bytes in, 1 + 4 + 4 K out.  Whether a tile touches a workgroup's block of
// pixels depends on blockIdx and the table alone, so the test is a scalar branch and a workgroup skips the tiles it does not touch
// (with 50 % overlap at most 4 of up to 64 touch a block away from the seams).  Two passes over the touching tiles: the first sums
// the weights (two table loads per tile, cached), the second loads the records.
// Loads: plain.  A workgroup is 4 rows of 64 pixels, a wave one row: its lanes read consecutive K-float records, a contiguous span
// of 64 K floats per tile that starts on any 4-byte boundary (K = 5; a tile may be a view), every byte of which is used.  No LDS,
// no barrier.  (Staging each tile's part of a 16 x 16 block through LDS as k_tta_merge does measured 30 % slower,
// profiles/window_notes.md: a wave's pixels are always one row of the tile here, there is nothing for LDS to straighten out.)
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int MAXK = SMSUT_TTA_MAX_CLASSES;
constexpr int MAXTILES = SMSUT_WINDOW_MAX_TILES;
constexpr int WIN_BW = 64, WIN_BH = TPB / WIN_BW;                          // a workgroup's block of pixels

struct WinTiles { const float* p[MAXTILES]; int ys[MAXTILES]; int xs[MAXTILES]; };

// KT > 0: the class count as a compile-time constant; KT = 0: a runtime K <= 32 under fully unrolled, guarded loops (static register
// indexing either way), as k_tta_merge.
template <int KT>
__global__ void __launch_bounds__(TPB)
k_window_blend(WinTiles tl, const float* __restrict__ wy, const float* __restrict__ wx, uint8_t* __restrict__ pred,
               float* __restrict__ conf, float* __restrict__ prob, int ny, int nx, int H, int W, int wh, int ww, int K) {
  constexpr int KK = KT ? KT : MAXK;
  if (KT) K = KT;
  const int n = blockIdx.z;
  const int by0 = blockIdx.y * WIN_BH, bx0 = blockIdx.x * WIN_BW;
  const int by1 = min(by0 + WIN_BH, H), bx1 = min(bx0 + WIN_BW, W);          // the block's pixels: [by0, by1) x [bx0, bx1)
  const int y = by0 + (int)threadIdx.x / WIN_BW, x = bx0 + (int)threadIdx.x % WIN_BW;
  const bool live = y < H && x < W;

  float s = 0.f;                                                           // pass 1: the sum of the covering tiles' weights
  for (int iy = 0; iy < ny; ++iy) {
    const int y0 = tl.ys[iy];
    if (y0 >= by1 || y0 + wh <= by0) continue;                             // (uniform per workgroup: a scalar branch)
    for (int ix = 0; ix < nx; ++ix) {
      const int x0 = tl.xs[ix];
      if (x0 >= bx1 || x0 + ww <= bx0) continue;
      if (live && y >= y0 && y < y0 + wh && x >= x0 && x < x0 + ww) {
        float w = wy[y - y0] * wx[x - x0];
        asm volatile("" : "+v"(w));                                        // the product is rounded on its own: no fma into s
        s += w;
      }
    }
  }

  float acc[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) acc[k] = 0.f;
  for (int iy = 0; iy < ny; ++iy) {                                        // pass 2: the records
    const int y0 = tl.ys[iy];
    if (y0 >= by1 || y0 + wh <= by0) continue;
    for (int ix = 0; ix < nx; ++ix) {
      const int x0 = tl.xs[ix];
      if (x0 >= bx1 || x0 + ww <= bx0) continue;
      const float* __restrict__ z = tl.p[iy * nx + ix];
      if (live && y >= y0 && y < y0 + wh && x >= x0 && x < x0 + ww) {
        float w = wy[y - y0] * wx[x - x0];
        asm volatile("" : "+v"(w));
        const float v = w / s;
        const float* row = z + (((int64_t)n * wh + (y - y0)) * ww + (x - x0)) * K;
#pragma unroll
        for (int k = 0; k < KK; ++k)
          if (k < K) acc[k] += v * row[k];
      }
    }
  }

  if (live) {
    const int64_t px = ((int64_t)n * H + y) * W + x;
    float best = acc[0];
    int arg = 0;
    if (prob) prob[px * K] = best;
#pragma unroll
    for (int k = 1; k < KK; ++k) {
      if (k < K) {
        const float v = acc[k];
        if (prob) prob[px * K + k] = v;
        if (v > best || (v != v && best == best)) { best = v; arg = k; }   // NaN wins, like torch (k_argmax_channels)
      }
    }
    pred[px] = (uint8_t)arg;
    if (conf) conf[px] = best;
  }
}

}  // namespace

extern "C" {

int smsut_window_blend(const float* const* tiles, const int* ys, const int* xs, const float* wy, const float* wx, uint8_t* pred,
                       float* conf, float* prob, int ny, int nx, int N, int H, int W, int wh, int ww, int K, void* stream) {
  SMSUT_REQUIRE(ny >= 1 && nx >= 1 && ny <= MAXTILES && nx <= MAXTILES && ny * nx <= MAXTILES && K >= 1 && K <= MAXK);
  SMSUT_REQUIRE(N >= 0 && N <= SMSUT_TTA_MAX_SLICES && H >= 1 && W >= 1 && H <= SMSUT_TTA_MAX_DIM && W <= SMSUT_TTA_MAX_DIM &&
                wh >= 1 && ww >= 1 && wh <= H && ww <= W);
  SMSUT_REQUIRE(tiles && ys && xs);
  WinTiles tl = {};
  for (int i = 0; i < ny; ++i) {                             // every tile inside the grid: no record outside a tile is addressed
    SMSUT_REQUIRE(ys[i] >= 0 && ys[i] <= H - wh);
    tl.ys[i] = ys[i];
  }
  for (int i = 0; i < nx; ++i) {
    SMSUT_REQUIRE(xs[i] >= 0 && xs[i] <= W - ww);
    tl.xs[i] = xs[i];
  }
  if (N == 0) return SMSUT_OK;
  SMSUT_REQUIRE(pred && wy && wx);
  for (int t = 0; t < ny * nx; ++t) {
    SMSUT_REQUIRE(tiles[t] && ((uintptr_t)tiles[t] & 3) == 0);
    tl.p[t] = tiles[t];
  }
  const dim3 grid((unsigned)((W + WIN_BW - 1) / WIN_BW), (unsigned)((H + WIN_BH - 1) / WIN_BH), (unsigned)N);
#define WIN_L(KT) k_window_blend<KT><<<grid, TPB, 0, (hipStream_t)stream>>>(tl, wy, wx, pred, conf, prob, ny, nx, H, W, wh, ww, K)
  switch (K) { case 2: WIN_L(2); break; case 3: WIN_L(3); break; case 4: WIN_L(4); break; case 5: WIN_L(5); break;
               default: WIN_L(0); }
#undef WIN_L
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

}  // extern "C"
