// Photometric augmentation on the device: ColorJitter(brightness, contrast) and RandomGammaCorrection of the reference's image
// transforms (data_loader/baseLoader.py:102-109, externalTransforms.py:23-43) on single-channel 8-bit slices, after the joint
// geometric passes and before Normalize.  Everything is per slice; no slice depends on a batchmate.
//
// The ops are PIL's, which work on 8-bit levels: brightness = blend(0, v, b), contrast = blend(m, v, c) with m the rounded mean
// of the slice AS IT IS when the contrast step runs, gamma = a 256-entry table.  Each is a map level -> level, so given the
// slice's histogram the whole chain is ONE 256-entry table per slice (the intermediate mean is sum hist[l] * cur[l] / count with
// cur the table built so far).  Two kernels:
//   k_photo_hist   histogram of the quantised levels; every workgroup writes its own row of part[N][G][256] (plain stores, no
//                  zeroing launch, no global atomics), the rows are summed in the next kernel's prologue;
//   k_photo_apply  prologue: 256 threads build the slice's table in LDS; body: quantise, look up, store.
// Integer adds only on the way to the table and IEEE fp32 steps in a fixed order inside it: the result is bit-reproducible and
// is held to bit equality with Pillow (tests/golden/photometric_pil.npz).
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int PHOTO_CHUNK = 4096;      // pixels a workgroup takes per slice before a slice gets another workgroup
constexpr int PHOTO_MAX_PARTS = 16;    // histogram workgroups per slice at most: every apply workgroup sums that many rows
constexpr int PHOTO_MAX_WGS = 64;      // apply workgroups per slice at most
constexpr int PHOTO_PREFETCH = 4;      // float4 loads the apply kernel issues before it builds the table

// PIL's blend is a rounded multiply followed by a rounded add.  The library is built with -ffp-contract=fast, which lets the
// backend fuse x * y + z into one fma wherever it sees the pair -- also when it is spelled __fadd_rn(__fmul_rn(x, y), z) (HIP's
// _rn intrinsics are plain operators) and also under `#pragma clang fp contract(off)` (the option is global to the code
// generator).  Passing the product through an empty asm statement hides its origin: no instruction, and nothing to fuse.
__device__ __forceinline__ float photo_rounded(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

inline int photo_wgs(int HW, int cap) {
  int g = (HW + PHOTO_CHUNK - 1) / PHOTO_CHUNK;
  return g < 1 ? 1 : (g > cap ? cap : g);
}
inline int photo_parts(int HW) { return photo_wgs(HW, PHOTO_MAX_PARTS); }

// The 8-bit level the reference's PIL image would hold for a value on the [0, 1] scale: floor(x * 255 + 0.5) clamped (PIL's
// rounding in resize, not round-half-even).  Multiply and add stay separate roundings.
// NaN -> 0 (fmaxf returns the other operand), so the result always indexes a 256-entry table.
__device__ __forceinline__ int photo_level(float x) {
  const float t = floorf(__fadd_rn(photo_rounded(__fmul_rn(x, 255.0f)), 0.5f));
  return (int)fminf(fmaxf(t, 0.0f), 255.0f);
}

// PIL's ImagingBlend of a constant image d with level v, factor a: fp32 multiply, fp32 add (no fma), truncation; clipped only when
// a lies outside [0, 1] (inside, the value cannot leave [0, 255]).
__device__ __forceinline__ int photo_blend(int d, int v, float a) {
  const float t = __fadd_rn((float)d, photo_rounded(__fmul_rn(a, (float)(v - d))));
  if (a >= 0.0f && a <= 1.0f) return (int)t;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// Where a slice's pixels go.  With 16-byte aligned base pointers the slice [n * HW, (n + 1) * HW) splits into `head` scalar
// pixels up to the next 16-byte boundary, nv float4 groups and a scalar tail; otherwise every pixel is a scalar one.
struct PhotoSplit { int head, nv, tail0, ns; };
__device__ __forceinline__ PhotoSplit photo_split(int n, int HW, int vec) {
  PhotoSplit s;
  s.head = vec ? min(HW, (4 - (int)(((int64_t)n * HW) & 3)) & 3) : 0;
  s.nv = vec ? (HW - s.head) >> 2 : 0;
  s.tail0 = s.head + 4 * s.nv;
  s.ns = s.head + (HW - s.tail0);                 // scalar pixels: [0, head) and [tail0, HW)
  return s;
}
__device__ __forceinline__ int photo_scalar_pixel(const PhotoSplit& s, int j) { return j < s.head ? j : s.tail0 + (j - s.head); }

// One level into the wave's LDS histogram.  Slices are mostly black background: 64 lanes adding to bin 0 serialise, so
// PHOTO_VOTE_ROUNDS values are taken out by vote first -- the lanes still holding a level read the first such lane's value
// (readfirstlane under the narrowed exec mask: scalar work, no LDS traffic), the ones that share it form one mask, and its first
// lane adds the popcount ONCE -- and only what is left goes through per-lane LDS atomics.  On full-range noise a round removes
// about one lane of 64 and is pure overhead, about as much as the rest of the kernel; measured with 0 to 3 rounds on noise and
// on 90 %-black slices (profiles/photometric_notes.md), ONE round is where the two regimes cost the same.
#ifndef PHOTO_VOTE_ROUNDS
#define PHOTO_VOTE_ROUNDS 1
#endif
__device__ __forceinline__ void photo_hist_add(int* h, int lv, bool valid) {
  const int lane = threadIdx.x & 63;
  bool rem = valid;
#pragma unroll
  for (int r = 0; r < PHOTO_VOTE_ROUNDS; ++r) {
    if (rem) {
      const int v = __builtin_amdgcn_readfirstlane(lv);
      if (lv == v) {
        const unsigned long long same = __ballot(1);          // the active lanes: exactly those that hold v
        if (lane == __ffsll((long long)same) - 1) atomicAdd(&h[v], (int)__popcll(same));
        rem = false;
      }
    }
  }
  if (rem) atomicAdd(&h[lv], 1);
}

__global__ void __launch_bounds__(TPB)
k_photo_hist(const float* __restrict__ img, int* __restrict__ part, int HW, int vec) {
  __shared__ int hw[4][256];                      // one histogram per wave
  const int n = blockIdx.y, g = blockIdx.x, G = gridDim.x, tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) hw[k][tid] = 0;
  __syncthreads();
  int* h = hw[tid >> 6];
  const float* src = img + (size_t)n * HW;
  const PhotoSplit s = photo_split(n, HW, vec);
  for (int v = g * TPB + tid; v < s.nv; v += G * TPB) {
    const float4 q = *reinterpret_cast<const float4*>(src + s.head + 4 * (size_t)v);
    photo_hist_add(h, photo_level(q.x), true);
    photo_hist_add(h, photo_level(q.y), true);
    photo_hist_add(h, photo_level(q.z), true);
    photo_hist_add(h, photo_level(q.w), true);
  }
  for (int j = g * TPB + tid; j < s.ns; j += G * TPB) photo_hist_add(h, photo_level(src[photo_scalar_pixel(s, j)]), true);
  __syncthreads();
  part[((size_t)n * G + g) * 256 + tid] = hw[0][tid] + hw[1][tid] + hw[2][tid] + hw[3][tid];
}

// params[n] = {order (0: brightness then contrast, 1: contrast then brightness), b, c, gamma drawn (0 / 1)}.
// part == null: no jitter (gamma only); gtab == null: no gamma.
__global__ void __launch_bounds__(TPB)
k_photo_apply(const float* __restrict__ img, const int* __restrict__ part, const float* __restrict__ params,
              const uint8_t* __restrict__ gtab, const float* __restrict__ out_tab, float* __restrict__ out, int HW, int parts,
              int vec) {
  __shared__ float lut[256];
  __shared__ double red[4];
  const int n = blockIdx.y, g = blockIdx.x, G = gridDim.x, tid = threadIdx.x;
  const float* src = img + (size_t)n * HW;
  float* dst = out + (size_t)n * HW;
  const PhotoSplit s = photo_split(n, HW, vec);
  // the first pixels are requested before the table exists: their latency hides under the prologue's chain of dependent loads
  float4 q[PHOTO_PREFETCH];
#pragma unroll
  for (int u = 0; u < PHOTO_PREFETCH; ++u) {
    const int v = (u * G + g) * TPB + tid;
    q[u] = v < s.nv ? *reinterpret_cast<const float4*>(src + s.head + 4 * (size_t)v) : make_float4(0.f, 0.f, 0.f, 0.f);
  }

  const float* p = params + (size_t)n * 4;
  int cur = tid;                                  // thread t carries level t through the chain
  if (part) {
    int cnt = 0;
    for (int k = 0; k < parts; ++k) cnt += part[((size_t)n * parts + k) * 256 + tid];
    const bool contrast_first = p[0] != 0.0f;
    const float b = p[1], c = p[2];
    if (!contrast_first) cur = photo_blend(0, cur, b);
    // the slice's mean as PIL takes it: int(S / count + 0.5) in fp64, S the integer sum of the levels as they are now.  The
    // products are integers below 2^31 * 255 and so is their sum: the fp64 additions are exact in any order.
    const double S = block_sum_256_d((double)cnt * (double)cur, red);
    const int m = (int)(S / (double)HW + 0.5);
    cur = photo_blend(m, cur, c);
    if (contrast_first) cur = photo_blend(0, cur, b);
  }
  if (gtab && p[3] != 0.0f) cur = gtab[(size_t)n * 256 + cur];
  lut[tid] = out_tab[cur];
  __syncthreads();

  auto put = [&](int v, const float4& a) {
    float4 r;
    r.x = lut[photo_level(a.x)]; r.y = lut[photo_level(a.y)]; r.z = lut[photo_level(a.z)]; r.w = lut[photo_level(a.w)];
    *reinterpret_cast<float4*>(dst + s.head + 4 * (size_t)v) = r;
  };
#pragma unroll
  for (int u = 0; u < PHOTO_PREFETCH; ++u) {
    const int v = (u * G + g) * TPB + tid;
    if (v < s.nv) put(v, q[u]);
  }
  for (int v = (PHOTO_PREFETCH * G + g) * TPB + tid; v < s.nv; v += G * TPB)
    put(v, *reinterpret_cast<const float4*>(src + s.head + 4 * (size_t)v));
  for (int j = g * TPB + tid; j < s.ns; j += G * TPB) {
    const int o = photo_scalar_pixel(s, j);
    dst[o] = lut[photo_level(src[o])];
  }
}

inline int aligned16(const void* a, const void* b) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

}  // namespace

extern "C" {

#define ST ((hipStream_t)stream)

int smsut_photo_parts(int HW) { return HW > 0 ? photo_parts(HW) : 0; }

int smsut_photo_hist(const float* img, int* part, int N, int HW, void* stream) {
  SMSUT_REQUIRE(img && part && N > 0 && N <= 65535 && HW > 0);
  hipLaunchKernelGGL(k_photo_hist, dim3(photo_parts(HW), N), dim3(TPB), 0, ST, img, part, HW, aligned16(img, img));
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

int smsut_photo_apply(const float* img, const int* part, const float* params, const uint8_t* gtab, const float* out_tab,
                      float* out, int N, int HW, void* stream) {
  SMSUT_REQUIRE(img && params && out_tab && out && out != img && N > 0 && N <= 65535 && HW > 0);
  hipLaunchKernelGGL(k_photo_apply, dim3(photo_wgs(HW, PHOTO_MAX_WGS), N), dim3(TPB), 0, ST, img, part, params, gtab, out_tab,
                     out, HW, photo_parts(HW), aligned16(img, out));
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

}  // extern "C"
