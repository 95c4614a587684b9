// What the kernels that read T member logit tensors on the un-transformed grid share (tta.hip: k_tta_merge; uncertainty.hip:
// k_tta_uncertain): the by-value member table, the position of a pixel under a transform, and the copy of one member's tile into
// LDS by member rows.  The access pattern and the LDS image layout are described at the top of tta.hip.
#pragma once
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int MAXT = SMSUT_TTA_MAX_MEMBERS;
constexpr int MAXK = SMSUT_TTA_MAX_CLASSES;
constexpr int STAGE_MAXC = 32;         // rows of up to this many channels go through LDS; longer rows are read in place
// Largest C that takes the 32 x 32 tile (a compile-time switch for the tile A/B of profiles/tta_notes.md: 0 = 16 x 16 everywhere).
#ifndef SMSUT_TTA_TILE32_MAXC
#define SMSUT_TTA_TILE32_MAXC 8
#endif
constexpr int TILE32_MAXC = SMSUT_TTA_TILE32_MAXC;

struct TtaMembers { const float* z[MAXT]; unsigned char g[MAXT]; };

// (a, b) = the position in F_g(x) of pixel (i, j) of x [H][W]
__device__ __forceinline__ void tta_pos(int g, int H, int W, int i, int j, int& a, int& b) {
  const int jf = (g & 4) ? W - 1 - j : j;
  switch (g & 3) {
    case 0: a = i; b = jf; break;
    case 1: a = W - 1 - jf; b = i; break;
    case 2: a = H - 1 - i; b = W - 1 - jf; break;
    default: a = jf; b = H - 1 - i; break;
  }
}

// One member's tile -- mh rows of mw pixels from (ma0, mb0) of slice n of z [N][H][W][C] -- into smem as
// smem[r * RS + px * CP + c], CP = C | 1, RS = TS * CP + 1; a barrier before the first write and one after the last.
// Called by all TPB threads of the workgroup.
template <int TS>
__device__ __forceinline__ void tta_stage_tile(float* smem, const float* __restrict__ z, int n, int H, int W, int C, int ma0, int mb0,
                                               int mh, int mw) {
  constexpr int LPR = 16, RPP = TPB / LPR;                   // staging: 16 lanes per member row, 16 rows per pass
  constexpr int PASSES = TS / RPP, UNR = 4;
  const int CP = C | 1, RS = TS * CP + 1;
  const int tx = threadIdx.x % LPR, ty = threadIdx.x / LPR;
  const int mis = (int)(((uintptr_t)z >> 2) & 3);            // floats of z past a 16-byte boundary
  const int len = mw * C;
  __syncthreads();                                           // the previous member's tile has been read
  for (int u0 = tx; u0 * 4 < len + 3; u0 += LPR * UNR) {     // (one round for TS * C <= 253 floats: every C <= 7 at TS = 32)
    float4 v[PASSES][UNR];
    int head[PASSES];
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
      const int r = ty + ps * RPP;
      const int64_t s = (((int64_t)n * H + ma0 + (r < mh ? r : 0)) * W + mb0) * C;   // first float of the row's span
      head[ps] = (int)((s + mis) & 3);                       // floats between the 16-byte boundary below the span and its start
      const float* src = z + (s - head[ps]);
#pragma unroll
      for (int q = 0; q < UNR; ++q) {
        const int i = (u0 + q * LPR) * 4;
        v[ps][q] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < mh && i < head[ps] + len) {
          if (i >= head[ps] && i + 4 <= head[ps] + len) {
            v[ps][q] = *(const float4*)(src + i);
          } else {
            float e[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (i + c >= head[ps] && i + c < head[ps] + len) e[c] = src[i + c];
            v[ps][q] = make_float4(e[0], e[1], e[2], e[3]);
          }
        }
      }
    }
#pragma unroll
    for (int ps = 0; ps < PASSES; ++ps) {
      const int r = ty + ps * RPP;
      float* dst = smem + r * RS;
#pragma unroll
      for (int q = 0; q < UNR; ++q) {
        const int j0 = (u0 + q * LPR) * 4 - head[ps];        // the span's float index of v.x
        const float e[4] = {v[ps][q].x, v[ps][q].y, v[ps][q].z, v[ps][q].w};
        if (r < mh) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int j = j0 + c;
            if (j >= 0 && j < len) {
              int o = j;
              if (CP != C) { const int px = (int)((unsigned)j / (unsigned)C); o = j + px; }   // px * CP + (j - px * C)
              dst[o] = e[c];
            }
          }
        }
      }
    }
  }
  __syncthreads();
}

inline bool tta_list_ok(const int* transforms, int T, int H, int W) {
  for (int t = 0; t < T; ++t) {
    const int g = transforms[t];
    if (g < 0 || g > 7 || ((g & 1) && H != W)) return false;
  }
  return true;
}

// The tile and staging choice of a launch (the table in include/smsut_hip.h): LDS-staged when C <= 32, 32 x 32 tiles with four
// pixels per lane when also C <= 8 and K is one of the compile-time class counts 2..5, else 16 x 16.
struct TtaTiling { bool staged, big; int ts; size_t tile_bytes; };
inline TtaTiling tta_tiling(int C, int K) {
  TtaTiling t;
  t.staged = C <= STAGE_MAXC;
  t.big = t.staged && C <= TILE32_MAXC && K >= 2 && K <= 5;
  t.ts = t.big ? 32 : 16;
  t.tile_bytes = t.staged ? (size_t)t.ts * (size_t)(t.ts * (C | 1) + 1) * sizeof(float) : 0;
  return t;
}

}  // namespace
