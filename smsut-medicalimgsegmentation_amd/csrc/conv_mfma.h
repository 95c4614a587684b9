// Internal: the device primitives and constants that conv_mfma.hip (forward / data-gradient) and conv_mfma_wgrad.hip (LDS-staged weight
// gradient) both use.  Everything sits in an anonymous namespace, so each file gets its own copy -- under -DSMSUT_STAMPS its own
// g_stamps buffer too, with a setter per file (smsut_dbg_set_stamps, smsut_dbg_wgrad_stamps).
#pragma once
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TPB = 256;
constexpr int TW = 16;       // pixels per MFMA M tile (one image row segment)

#ifdef SMSUT_STAMPS   // diagnostic build only (scratch/ubench/stamps.py): wave timeline via s_memtime, MICROARCH "In-kernel stamps"
__device__ unsigned long long* g_stamps = nullptr;      // [512 workgroups][4 waves][16]
__device__ int g_stamp_base = 0;                        // first workgroup (blockIdx.x) recorded
#define STAMP(i)                                                                                       \
  if (g_stamps && lane == 0 && stamp_wg >= g_stamp_base && stamp_wg < g_stamp_base + 512)                \
    g_stamps[(((stamp_wg - g_stamp_base) * 4 + wave) * 16) + (i)] = __builtin_amdgcn_s_memtime();
#else
#define STAMP(i)
#endif

__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ---- fp16-operand mode (BASELINE config 5: 512x512 slices, "fp16 MFMA conv path with fp32 IN / loss accumulators") ----------
// Tensors stay fp32 in HBM; a kernel instantiated with F16 converts its operands to fp16 WHILE STAGING them into LDS and
// multiplies with v_mfma_f32_16x16x16_f16 -- one instruction per 16-channel chunk and tap instead of four fp32 ones, fp32
// accumulators, statistics, epilogues and outputs unchanged (the C/D register layout is dtype-independent on gfx950).
// LDS images: input tile [pixel][24 halves] (16 used; 48-B pixel stride makes the ds_read_b64 of lane (pixel lm, 4kq..4kq+3)
// conflict-free: banks 12*lm + 2*kq + {0,1} are all distinct within a 32-lane half), weights [tap][chunk][n][24 halves].
// Gradient operands (gy of the data- and weight-gradient passes) would underflow fp16 (|gy| ~ 1e-7 at 512^2): the caller
// passes gsc = {s, 1/s}, a per-tensor power-of-two scale from smsut_absmax_scale; gy*s is what is converted, the fp32
// result is multiplied by 1/s -- exact, no loss-scale bookkeeping outside the kernel.
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 mfma16h(h4 a, h4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
}
// gfx950's double-depth instruction (r05): v_mfma_f32_16x16x32_f16, 32 k-slots per issue.  A 16-channel chunk fills 16 of them, so the
// forward kernels feed it TWO TAPS at a time: k-slots 0..15 = the chunk's channels under tap 2p, 16..31 = under tap 2p+1.  Lane
// (lm, kq) holds k = 8kq .. 8kq+7, i.e. eight consecutive channels of ITS tap (kq >> 1): one ds_read_b128 per fragment instead of two
// ds_read_b64, one MFMA issue instead of two; the 48-B pixel stride keeps eight consecutive lanes on 32 distinct banks.  A lone tap
// (the ninth of a 3x3 conv, a 1x1 conv, the centre tap of the fused shortcut data-gradient's second half) runs the SAME instruction
// with the upper sixteen k-slots multiplying zeros -- it holds the pipe as long as the 16-deep one, and the two must not be mixed on one
// accumulator: a v_mfma_f32_16x16x16_f16 accumulating onto a register a v_mfma_f32_16x16x32_f16 had just written DROPPED that
// contribution (statistics form, 16 -> 16, rows 4r+2 / columns 4q, 4q+1 of every tile: scratch/x32_debug.py; the dependent issue came
// too early).  The weight gradient pairs two tile ROWS per issue.  SMSUT_F16_X32=0 at compile time: 16-deep instructions throughout.
#ifndef SMSUT_F16_X32
#define SMSUT_F16_X32 1
#endif
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x4 mfma32h(h8 a, h8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ h4 to_h4(float4 v) { return (h4){(_Float16)v.x, (_Float16)v.y, (_Float16)v.z, (_Float16)v.w}; }

// input-side InstanceNorm + LeakyReLU of the INAFF forms (conv_mfma_fwd_p): the same in_affine() fma as norm.hip, the same bits
__device__ __forceinline__ float aff1(float v, float m, float r, float g, float b, float slope) {
  return lrelu_f(in_affine(v, m, r, g, b), slope);
}

}  // namespace
