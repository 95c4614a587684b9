// Validation on the device: the argmax of a batch of logits and the three integers per (volume, class) that the Dice matrix needs,
// in one pass over the logits as they leave the network (misc/utils.py: DiceCounter; trainer/baseTrainer.py: validate_epoch_device).
//   counts[V][K][3] += {|P & G|, |P|, |G|}   (int64, ACCUMULATED: the caller zeroes it once per validation)
//   pred[N][HW] = argmax as a byte (optional)
// Integers only: per-thread register counters, a wave and block reduction, then one 64-bit integer atomicAdd per non-zero
// (class, statistic) and workgroup -- sums of integers do not depend on the order, so the result is bitwise reproducible.
// Logits are NHWC [N][HW][C]; labels int64 [N][HW]; the prediction is the first maximum of channels 0 .. K-1 (K <= C, K <= 32),
// by the comparison of k_argmax_channels (loss.hip): the first maximum wins, a NaN wins.
#include "common.h"

namespace {
constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MAXC = 32;           // classes (as loss.hip)
constexpr int STAGE_MAXC = 32;     // rows of up to this many channels go through LDS (36 KB at 32); longer rows are read in place
// Workgroups per slice at most, each flushing <= 3 K atomics onto ONE row of counts (24 * K bytes).  Measured at 8 x 256 x 256 x 5
// (back-to-back launches, profiles/validation_notes.md): 32 -> 13.0 us, 64 -> 12.9 us, 128 -> 17.4 us, 256 -> 28.8 us: past 64 the
// atomics on that one row cost more than the extra workgroups hide.  (A compile-time switch, for that A/B only.)
#ifndef SMSUT_EVAL_SLICE_BLOCKS
#define SMSUT_EVAL_SLICE_BLOCKS 64
#endif
constexpr int SLICE_BLOCKS = SMSUT_EVAL_SLICE_BLOCKS;

// One workgroup serves 256-pixel tiles of ONE slice (blockIdx.y = n), so all its counts go to one volume.
// STAGED: a tile's rows are one contiguous span of 256 * C floats.  With C = 5 a lane reading its own 20-byte row issues five
// strided dwords (the form loss.hip:17 measured at 1.2 TB/s); here the wave copies the span to LDS with 16-byte loads -- the span
// starts anywhere (n * HW * C need not be a multiple of 4), so the copy starts at the 16-byte boundary below it and the up to three
// floats in front of the span and behind it are skipped element by element, never read -- and each lane then reads its row from
// LDS (stride C dwords: conflict-free for odd C).  !STAGED (C > 32): the K <= 32 leading floats of each long row, in place.
// KT > 0: the class count as a compile-time constant, counters in registers (no dynamic indexing).  KT = 0: a runtime loop over
// the classes in which the wave VOTES (ballot + popcount) and its first lane adds to the wave's own LDS row: no per-lane LDS
// atomics on the class word -- on a segmentation nearly every lane holds class 0.
template <int KT, bool STAGED>
__global__ void __launch_bounds__(TPB)
k_eval_overlap(const float* __restrict__ logits, const int64_t* __restrict__ labels, const int* __restrict__ vol,
               unsigned long long* __restrict__ counts, uint8_t* __restrict__ pred, int64_t HW, int C, int K, int V) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int n = blockIdx.y;
  const int v = vol[n];
  if (v < 0 || v >= V) return;                                // (uniform) a slice of no volume: nothing counted, pred untouched
  if (KT) K = KT;
  const int tile_floats = STAGED ? ((TPB * C + 8 + 3) & ~3) : 0;
  unsigned long long* hist = (unsigned long long*)(smem + tile_floats);      // [WAVES][K][3]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long* h = hist + (size_t)wave * K * 3;
  constexpr int KK = KT ? KT : 1;
  unsigned ci[KK], cp[KK], cg[KK];
#pragma unroll
  for (int k = 0; k < KK; ++k) { ci[k] = 0; cp[k] = 0; cg[k] = 0; }
  if (!KT) {
    for (int i = threadIdx.x; i < WAVES * K * 3; i += TPB) hist[i] = 0;
    __syncthreads();
  }
  const int mis = (int)(((uintptr_t)logits >> 2) & 3);         // floats of `logits` past a 16-byte boundary
  const int64_t ntiles = (HW + TPB - 1) / TPB;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {          // (uniform: barriers inside)
    const int64_t p0 = tile * TPB;
    const int npx = (int)(HW - p0 < TPB ? HW - p0 : TPB);
    const int64_t s = ((int64_t)n * HW + p0) * C;              // first float of the tile's span
    const bool valid = (int)threadIdx.x < npx;
    const int64_t px = (int64_t)n * HW + p0 + threadIdx.x;
    const int64_t g = valid ? labels[px] : -1;                 // (issued before the staging: one memory latency per tile, not two)
    int row = 0;
    if (STAGED) {
      const int len = npx * C;
      const int head = (int)((s + mis) & 3);                   // floats between the 16-byte boundary below the span and its start
      __syncthreads();                                         // the previous tile's rows have been read
      for (int i = threadIdx.x * 4; i < head + len; i += TPB * 4) {
        if (i >= head && i + 4 <= head + len) {
          *(float4*)(smem + i) = *(const float4*)(logits + (s - head + i));
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (i + j >= head && i + j < head + len) smem[i + j] = logits[s - head + i + j];
        }
      }
      __syncthreads();
      row = head + threadIdx.x * C;
    }
    int p = 0;
    if (valid) {
      auto at = [&](int c) -> float {
        if constexpr (STAGED) return smem[row + c];
        else return logits[s + (int64_t)threadIdx.x * C + c];
      };
      float best = at(0);
#pragma unroll
      for (int c = 1; c < (KT ? KT : K); ++c) {
        const float z = at(c);
        if (z > best || (z != z && best == best)) { best = z; p = c; }        // NaN wins, like torch (k_argmax_channels)
      }
      if (pred) pred[px] = (uint8_t)p;
    }
    if (KT) {
#pragma unroll
      for (int k = 0; k < KK; ++k) {
        const int ip = valid && p == k, ig = valid && g == (int64_t)k;
        cp[k] += ip; cg[k] += ig; ci[k] += ip & ig;
      }
    } else {
      for (int k = 0; k < K; ++k) {
        const bool ip = valid && p == k, ig = valid && g == (int64_t)k;
        const unsigned long long mp = __ballot(ip), mg = __ballot(ig), mi = __ballot(ip && ig);
        if (lane == 0) { h[k * 3] += __popcll(mi); h[k * 3 + 1] += __popcll(mp); h[k * 3 + 2] += __popcll(mg); }
      }
    }
  }
  if (KT) {
    // wave sums, step by step over ALL 3 K counters (their shuffles in flight together: summed one counter after the other the
    // 3 K x 6 dependent shuffles were ~110 LDS round trips in every workgroup's tail).  32 bits hold a wave's sum: 64 lanes x
    // the tiles of a workgroup, below 2^32 for any HW < 2^40; across waves and workgroups the sums are 64-bit.
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      unsigned ti[KK], tp[KK], tg[KK];
#pragma unroll
      for (int k = 0; k < KK; ++k) { ti[k] = __shfl_xor(ci[k], o, 64); tp[k] = __shfl_xor(cp[k], o, 64); tg[k] = __shfl_xor(cg[k], o, 64); }
#pragma unroll
      for (int k = 0; k < KK; ++k) { ci[k] += ti[k]; cp[k] += tp[k]; cg[k] += tg[k]; }
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < KK; ++k) { h[k * 3] = ci[k]; h[k * 3 + 1] = cp[k]; h[k * 3 + 2] = cg[k]; }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * 3; i += TPB) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += hist[(size_t)w * K * 3 + i];
    if (t) atomicAdd(counts + (size_t)v * K * 3 + i, t);
  }
}

}  // namespace

extern "C" {

int smsut_eval_overlap(const float* logits, const int64_t* labels, const int* vol, int64_t* counts, uint8_t* pred, int N,
                       int64_t HW, int C, int K, int V, void* stream) {
  SMSUT_REQUIRE(N >= 0 && N <= 65535 && K >= 1 && K <= C && K <= MAXC && HW >= 1 && V >= 1);
  if (N == 0) return SMSUT_OK;
  SMSUT_REQUIRE(logits && labels && vol && counts);
  const int64_t ntiles = cdiv64(HW, TPB);
  const dim3 grid((unsigned)(ntiles < SLICE_BLOCKS ? ntiles : SLICE_BLOCKS), (unsigned)N);
  const bool staged = C <= STAGE_MAXC;
  const size_t lds = (staged ? (size_t)((TPB * C + 8 + 3) & ~3) * sizeof(float) : 0) + (size_t)WAVES * K * 3 * sizeof(unsigned long long);
#define EVAL_L(KT, ST) k_eval_overlap<KT, ST><<<grid, TPB, lds, (hipStream_t)stream>>>(logits, labels, vol, (unsigned long long*)counts, \
                                                                                 pred, HW, C, K, V)
#define EVAL_K(KT) do { if (staged) EVAL_L(KT, true); else EVAL_L(KT, false); } while (0)
  switch (K) { case 2: EVAL_K(2); break; case 3: EVAL_K(3); break; case 4: EVAL_K(4); break; case 5: EVAL_K(5); break;
               default: EVAL_K(0); }
#undef EVAL_K
#undef EVAL_L
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

}  // extern "C"
