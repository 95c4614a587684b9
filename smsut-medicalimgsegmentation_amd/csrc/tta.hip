// Test-time augmentation and ensembling on the device (smsut_amd/predict.py): the network sees flipped / rotated copies of a slice,
// the class probabilities of all copies (and of all networks of an ensemble) are averaged on the un-transformed grid, and the label
// and a confidence are taken from the mean.
//
// The eight transforms (the ONE definition; ops.tta_transforms and tests/tta_ref.py state the same in torch): g = r + 4 f,
//   F_g(x) = rot90(f ? flip(x, last axis) : x, k = r) on the last two axes, counter-clockwise as torch.rot90.
// With jf = f ? W - 1 - j : j, pixel (i, j) of x sits in F_g(x) at
//   r = 0: (i, jf)     r = 1: (W - 1 - jf, i)     r = 2: (H - 1 - i, W - 1 - jf)     r = 3: (jf, H - 1 - i)
// (tta_pos below); odd r needs H == W.
//
// k_tta_expand: uint8 slices [N][H][W] -> fp32 [T][N][1][H][W], member t = F_{g_t}(slice) converted as the loader converts it on
//   the device, ((float)u * (float)(1.0 / 255.0) - 0.5f) * 2.0f, each step rounded to fp32 (the bits of torch's
//   `.float().div(255).sub(.5).div(.5)` on a device tensor).  One output element per thread: coalesced stores, byte gathers from
//   a source that stays in cache.
// k_tta_merge: T member logit tensors [N][H][W][C] (NHWC, each read in place through its own base pointer: a by-value table in the
//   kernel arguments, nothing is stacked or copied) -> pred uint8 [N][H][W], optional conf fp32 [N][H][W], optional prob fp32
//   [N][H][W][K].  Per output pixel q, member by member in list order: p = F_g(q); m = max_k z[p][k]; e_k = expf(z[p][k] - m);
//   s = e_0 + e_1 + ... in channel order; acc_k += e_k / s.  Then mean_k = acc_k / (float)T, pred = the first maximum of mean_k by
//   k_argmax_channels' comparison (the first maximum wins, a NaN wins), conf = mean_pred.  A pixel belongs to one lane from its
//   first load to its stores: no atomics, no cross-lane sums, so two calls are bitwise equal.
//
// Access pattern of the merge.  A square output tile maps to a square member tile under all eight transforms, so a workgroup
// stages each member's tile through LDS BY MEMBER ROWS -- contiguous spans of (tile width) * C floats whatever g is -- and each
// lane then picks its transformed pixel from LDS.  A span starts on any 4-byte boundary (C = 5; a member may be a view that starts
// anywhere in its allocation), so a row is copied from the 16-byte boundary below its start in 16-byte units, and the up to three
// floats in front of the span and behind it are skipped element by element, never read (as k_eval_overlap does).  The units of up
// to 2 x 4 rows per lane are loaded before the first is stored: 8 x 16 bytes in flight per lane.  LDS is written dword by dword
// (four ds_write_b32 cost what one ds_write_b128 costs on this chip), which leaves the image layout free:
//   pixel stride CP = C | 1 dwords, row stride RS = TS * CP + 1 dwords, both odd.
// Even r: the lanes of a wave read consecutive pixels of a row, stride CP -- conflict-free because CP is odd (for an even C the
// pixel rows are padded by one dword; that costs one integer division per staged float, paid only by even C).  Odd r: consecutive
// lanes read consecutive ROWS, stride RS -- conflict-free because RS is odd.
// Tile: 32 x 32 with four pixels per lane when C <= 8 and K is one of the compile-time class counts (640-byte spans at C = 5, 20 KB
// of LDS), else 16 x 16 with one pixel per lane (the accumulators of 32 runtime classes times four pixels would not fit the
// register budget, and 32 rows of 32 x 33 floats would not fit LDS).  C > 32: the K <= 32 leading floats of each long row are read
// in place, as evaluate.hip does.  The member table, tta_pos and the staging copy live in tta_stage.h, which k_tta_uncertain
// (uncertainty.hip) shares.
#include "tta_stage.h"

namespace {
struct TtaList { unsigned char g[MAXT]; };

__global__ void __launch_bounds__(TPB)
k_tta_expand(const uint8_t* __restrict__ img, float* __restrict__ out, TtaList list, int64_t total, int N, int H, int W) {
  const int64_t hw = (int64_t)H * W;
  for (int64_t idx = (int64_t)blockIdx.x * TPB + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * TPB) {
    const int64_t tn = idx / hw;
    const int rem = (int)(idx - tn * hw);
    const int a = rem / W, b = rem - a * W;                  // (a member of an odd r is W x H = H x W: the same strides)
    const int t = (int)(tn / N), n = (int)(tn - (int64_t)t * N);
    const int g = list.g[t];
    int i, jf;                                               // the inverse of tta_pos
    switch (g & 3) {
      case 0: i = a; jf = b; break;
      case 1: i = b; jf = W - 1 - a; break;
      case 2: i = H - 1 - a; jf = W - 1 - b; break;
      default: i = H - 1 - b; jf = a; break;
    }
    const int j = (g & 4) ? W - 1 - jf : jf;
    const float u = (float)img[(int64_t)n * hw + (int64_t)i * W + j];
    // data_loader/inTurnLoader.py:166,173 -- `.float().div_(255.0).sub_(0.5).div_(0.5)` ON THE DEVICE, where torch divides by a
    // host scalar as a multiplication by its reciprocal, (float)(1.0 / 255.0) and 2.0f; every step rounded on its own: the
    // empty asm makes the product opaque, so that -ffp-contract=fast (which the backend applies whatever a pragma says)
    // cannot fuse it into the subtraction
    float p = u * (float)(1.0 / 255.0);
    asm volatile("" : "+v"(p));
    out[idx] = (p - 0.5f) * 2.0f;
  }
}

// KT > 0: the class count as a compile-time constant; KT = 0: a runtime K <= 32 under fully unrolled, guarded loops (static register
// indexing either way).  PPL: pixels per lane, 4 = the 32 x 32 tile, 1 = 16 x 16.  STAGED: member tiles go through LDS.
template <int KT, int PPL, bool STAGED>
__global__ void __launch_bounds__(TPB)
k_tta_merge(TtaMembers mem, uint8_t* __restrict__ pred, float* __restrict__ conf, float* __restrict__ prob, int T, int H, int W, int C,
            int K) {
  constexpr int TS = PPL == 4 ? 32 : 16;
  constexpr int KK = KT ? KT : MAXK;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (KT) K = KT;
  const int n = blockIdx.z;
  const int oy0 = blockIdx.y * TS, ox0 = blockIdx.x * TS;
  const int th = min(TS, H - oy0), tw = min(TS, W - ox0);
  const int CP = C | 1, RS = TS * CP + 1;
  const int lx = threadIdx.x % TS, ly = threadIdx.x / TS;    // this lane's pixels: (oy0 + ly + p * (TPB / TS), ox0 + lx)
  float acc[PPL][KK];
#pragma unroll
  for (int p = 0; p < PPL; ++p)
#pragma unroll
    for (int k = 0; k < KK; ++k) acc[p][k] = 0.f;

  for (int t = 0; t < T; ++t) {                              // (uniform: barriers inside)
    const float* __restrict__ z = mem.z[t];
    const int g = mem.g[t];
    int a0, b0, a1, b1;                                      // the member's tile: the image of the output tile's corners
    tta_pos(g, H, W, oy0, ox0, a0, b0);
    tta_pos(g, H, W, oy0 + th - 1, ox0 + tw - 1, a1, b1);
    const int ma0 = min(a0, a1), mb0 = min(b0, b1);
    const int mh = (g & 1) ? tw : th, mw = (g & 1) ? th : tw;
    if (STAGED) tta_stage_tile<TS>(smem, z, n, H, W, C, ma0, mb0, mh, mw);
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
      const int oy = ly + p * (TPB / TS), ox = lx;
      if (oy < th && ox < tw) {
        int a, b;
        tta_pos(g, H, W, oy0 + oy, ox0 + ox, a, b);
        const float* row = STAGED ? smem + (a - ma0) * RS + (b - mb0) * CP : z + (((int64_t)n * H + a) * W + b) * C;
        float e[KK];
#pragma unroll
        for (int k = 0; k < KK; ++k) e[k] = k < K ? row[k] : 0.f;
        float m = e[0];
#pragma unroll
        for (int k = 1; k < KK; ++k)
          if (k < K) m = fmaxf(m, e[k]);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < KK; ++k)
          if (k < K) { e[k] = expf(e[k] - m); s = k ? s + e[k] : e[k]; }
#pragma unroll
        for (int k = 0; k < KK; ++k)
          if (k < K) acc[p][k] += e[k] / s;
      }
    }
  }

  const float tf = (float)T;
#pragma unroll
  for (int p = 0; p < PPL; ++p) {
    const int oy = ly + p * (TPB / TS), ox = lx;
    if (oy < th && ox < tw) {
      const int64_t px = ((int64_t)n * H + oy0 + oy) * W + ox0 + ox;
      float best = acc[p][0] / tf;
      int arg = 0;
      if (prob) prob[px * K] = best;
#pragma unroll
      for (int k = 1; k < KK; ++k) {
        if (k < K) {
          const float v = acc[p][k] / tf;
          if (prob) prob[px * K + k] = v;
          if (v > best || (v != v && best == best)) { best = v; arg = k; }     // NaN wins, like torch (k_argmax_channels)
        }
      }
      pred[px] = (uint8_t)arg;
      if (conf) conf[px] = best;
    }
  }
}

}  // namespace

extern "C" {

int smsut_tta_expand(const uint8_t* img, float* out, const int* transforms, int T, int N, int H, int W, void* stream) {
  SMSUT_REQUIRE(T >= 1 && T <= MAXT && N >= 0 && N <= SMSUT_TTA_MAX_SLICES && H >= 1 && W >= 1 && H <= SMSUT_TTA_MAX_DIM &&
                W <= SMSUT_TTA_MAX_DIM);
  SMSUT_REQUIRE(transforms && tta_list_ok(transforms, T, H, W));
  if (N == 0) return SMSUT_OK;
  SMSUT_REQUIRE(img && out);
  TtaList list = {};
  for (int t = 0; t < T; ++t) list.g[t] = (unsigned char)transforms[t];
  const int64_t total = (int64_t)T * N * H * W;
  k_tta_expand<<<ew_grid(total, TPB), TPB, 0, (hipStream_t)stream>>>(img, out, list, total, N, H, W);
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

int smsut_tta_merge(const float* const* members, const int* transforms, uint8_t* pred, float* conf, float* prob, int T, int N, int H,
                    int W, int C, int K, void* stream) {
  SMSUT_REQUIRE(T >= 1 && T <= MAXT && N >= 0 && N <= SMSUT_TTA_MAX_SLICES && H >= 1 && W >= 1 && H <= SMSUT_TTA_MAX_DIM &&
                W <= SMSUT_TTA_MAX_DIM && K >= 1 && K <= C && K <= MAXK);
  SMSUT_REQUIRE(members && transforms && tta_list_ok(transforms, T, H, W));
  if (N == 0) return SMSUT_OK;
  SMSUT_REQUIRE(pred);
  TtaMembers mem = {};
  for (int t = 0; t < T; ++t) {
    SMSUT_REQUIRE(members[t] && ((uintptr_t)members[t] & 3) == 0);
    mem.z[t] = members[t];
    mem.g[t] = (unsigned char)transforms[t];
  }
  const TtaTiling tl = tta_tiling(C, K);
  const bool staged = tl.staged, big = tl.big;
  const dim3 grid((unsigned)((W + tl.ts - 1) / tl.ts), (unsigned)((H + tl.ts - 1) / tl.ts), (unsigned)N);
  const size_t lds = tl.tile_bytes;
#define TTA_L(KT, PPL, ST) k_tta_merge<KT, PPL, ST><<<grid, TPB, lds, (hipStream_t)stream>>>(mem, pred, conf, prob, T, H, W, C, K)
#define TTA_K(KT) do { if (big) TTA_L(KT, 4, true); else if (staged) TTA_L(KT, 1, true); else TTA_L(KT, 1, false); } while (0)
  switch (K) { case 2: TTA_K(2); break; case 3: TTA_K(3); break; case 4: TTA_K(4); break; case 5: TTA_K(5); break;
               default: if (staged) TTA_L(0, 1, true); else TTA_L(0, 1, false); }
#undef TTA_K
#undef TTA_L
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

}  // extern "C"
