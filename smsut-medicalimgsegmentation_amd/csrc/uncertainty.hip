// Uncertainty of a test-time-augmented / ensembled prediction, in the merge's own pass over the T member logit tensors
// (smsut_amd/predict.py: Predictor.predict_uncertain; ops.tta_uncertainty; misc/utils.py: structure_agreement).
//
// k_tta_uncertain reads what k_tta_merge (tta.hip) reads, the same way -- same tiles, same staging through LDS (tta_stage.h), same
// softmax and accumulation, so pred and conf are bitwise the merge's -- and keeps, per pixel, a little more state in registers:
//   per member t in list order:  z = member[F_g(q)][0..K-1];  a_t = the first maximum of z (k_argmax_channels' comparison: the
//     first maximum wins, a NaN wins);  m = max_k z_k;  e_k = expf(z_k - m);  s = e_0 + e_1 + ... in channel order;  q_k = e_k / s;
//     acc_k += q_k;  h_t = -(q_0 logf(q_0 + 1e-6f) + q_1 logf(q_1 + 1e-6f) + ...) in channel order;  hs += h_t
//   then:  mean_k = acc_k / (float)T;  pred = the first maximum of mean;  conf = mean_pred;
//     H = -(mean_0 logf(mean_0 + 1e-6f) + ...) in channel order (the predictive entropy; the arithmetic of tests/uamt_ref.py);
//     EH = hs / (float)T;  MI = fmaxf(H - EH, 0.f) (the mutual information, BALD);  votes = #{t : a_t == pred}.
// Every product q logf(q + 1e-6f) is rounded on its own before it is added (an empty asm keeps -ffp-contract=fast from fusing it),
// so h_t of one member and H of a one-member mean are the same bits and MI is exactly 0 at T = 1.
// Per pixel the member labels are kept packed, 5 bits each, six to a 32-bit word (three words at T = 16), next to the 32-bit set
// of classes the members chose; votes and the per-member counts are resolved from them once pred is known.
//
// counts int64 [K][2 T + 4] (optional, ADDED into: the caller zeroes it once per volume), row k =
//   {V, ALL, ANY, HSUM, V_0 .. V_{T-1}, I_0 .. I_{T-1}}:  V: pixels with pred == k;  ALL: every a_t == k;  ANY: some a_t == k;
//   V_t: a_t == k;  I_t: a_t == k and pred == k;  HSUM: the sum over pixels with pred == k of (int64)rintf(H * 1048576.f) -- the
//   scaling by 2^20 is exact, so HSUM is a sum of integers; a pixel whose H is not finite adds nothing to it (and counts everywhere
//   else).
// Integers only, as evaluate.hip counts: each wave VOTES (ballot + popcount) per class that occurs in it -- a wave of a
// segmentation holds one to three classes, so the loop over classes is over those -- and adds its counts to the workgroup's
// 64-bit counters in LDS: lane i of the wave carries slot i of the class's row, so a row is ONE LDS atomic instruction.  HSUM is a
// wave sum of 32-bit integers by shuffles.  After a barrier the workgroup issues one 64-bit integer
// atomicAdd per non-zero counter.  Sums of integers do not depend on the order: two calls are bitwise equal.
#include "tta_stage.h"

namespace {
constexpr int LAB_BITS = 5, LAB_PER = 6, LAB_WORDS = (MAXT + LAB_PER - 1) / LAB_PER;   // member labels: six to a 32-bit word
constexpr float H_SCALE = 1048576.f;                          // 2^20
enum { SLOT_V = 0, SLOT_ALL = 1, SLOT_ANY = 2, SLOT_HSUM = 3, SLOT_VT = 4 };

struct UncertainOut { uint8_t* pred; float* conf; float* entropy; float* mutual; uint8_t* votes; unsigned long long* counts; };

// -(q_0 logf(q_0 + 1e-6f) + q_1 logf(q_1 + 1e-6f) + ...), every product rounded on its own
template <int KK>
__device__ __forceinline__ float entropy_of(const float (&q)[KK], int K) {
  float h = 0.f;
#pragma unroll
  for (int k = 0; k < KK; ++k) {
    if (k < K) {
      float pr = q[k] * logf(q[k] + 1e-6f);
      asm volatile("" : "+v"(pr));
      h = k ? h + pr : pr;
    }
  }
  return -h;
}

// the label of member t (a compile-time constant wherever this is called from an unrolled loop: a static register, one v_bfe_u32)
__device__ __forceinline__ unsigned label_at(const unsigned (&lab)[LAB_WORDS], int t) {
  return (lab[t / LAB_PER] >> (LAB_BITS * (t % LAB_PER))) & 31u;
}

// KT, PPL, STAGED: as k_tta_merge
template <int KT, int PPL, bool STAGED>
__global__ void __launch_bounds__(TPB)
k_tta_uncertain(TtaMembers mem, UncertainOut out, int T, int H, int W, int C, int K, int tile_floats) {
  constexpr int TS = PPL == 4 ? 32 : 16;
  constexpr int KK = KT ? KT : MAXK;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (KT) K = KT;
  const int n = blockIdx.z;
  const int oy0 = blockIdx.y * TS, ox0 = blockIdx.x * TS;
  const int th = min(TS, H - oy0), tw = min(TS, W - ox0);
  const int CP = C | 1, RS = TS * CP + 1;
  const int lx = threadIdx.x % TS, ly = threadIdx.x / TS;    // this lane's pixels: (oy0 + ly + p * (TPB / TS), ox0 + lx)
  const int slots = 2 * T + SLOT_VT;
  unsigned long long* cnt = (unsigned long long*)(smem + tile_floats);          // [K][slots], the workgroup's counters
  const bool want_mi = out.mutual != nullptr;                // (uniform) the per-member entropies serve the mutual information only
  if (out.counts) {
    for (int i = threadIdx.x; i < K * slots; i += TPB) cnt[i] = 0;
    __syncthreads();
  }
  float acc[PPL][KK], hs[PPL];
  unsigned lab[PPL][LAB_WORDS], seen[PPL];
#pragma unroll
  for (int p = 0; p < PPL; ++p) {
    hs[p] = 0.f; seen[p] = 0;
#pragma unroll
    for (int i = 0; i < LAB_WORDS; ++i) lab[p][i] = 0;
#pragma unroll
    for (int k = 0; k < KK; ++k) acc[p][k] = 0.f;
  }

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
        float m = e[0], best = e[0];
        unsigned arg = 0;
#pragma unroll
        for (int k = 1; k < KK; ++k) {
          if (k < K) {
            m = fmaxf(m, e[k]);
            if (e[k] > best || (e[k] != e[k] && best == best)) { best = e[k]; arg = k; }   // NaN wins (k_argmax_channels)
          }
        }
        seen[p] |= 1u << arg;
#pragma unroll
        for (int i = 0; i < LAB_WORDS; ++i)                   // (t is uniform: a scalar branch, a static register)
          if (t / LAB_PER == i) lab[p][i] |= arg << (LAB_BITS * (t % LAB_PER));
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < KK; ++k)
          if (k < K) { e[k] = expf(e[k] - m); s = k ? s + e[k] : e[k]; }
#pragma unroll
        for (int k = 0; k < KK; ++k)
          if (k < K) { e[k] = e[k] / s; acc[p][k] += e[k]; }
        if (want_mi) hs[p] += entropy_of<KK>(e, K);
      }
    }
  }

  const float tf = (float)T;
  bool valid[PPL];
  unsigned pr[PPL];
  int hq[PPL];                                               // rintf(H * 2^20), 0 where H is not finite
#pragma unroll
  for (int p = 0; p < PPL; ++p) {
    const int oy = ly + p * (TPB / TS), ox = lx;
    valid[p] = oy < th && ox < tw;
    pr[p] = 0; hq[p] = 0;
    if (valid[p]) {
      const int64_t px = ((int64_t)n * H + oy0 + oy) * W + ox0 + ox;
      float mean[KK];
#pragma unroll
      for (int k = 0; k < KK; ++k) mean[k] = k < K ? acc[p][k] / tf : 0.f;
      float best = mean[0];
      unsigned arg = 0;
#pragma unroll
      for (int k = 1; k < KK; ++k)
        if (k < K && (mean[k] > best || (mean[k] != mean[k] && best == best))) { best = mean[k]; arg = k; }
      pr[p] = arg;
      out.pred[px] = (uint8_t)arg;
      if (out.conf) out.conf[px] = best;
      if (out.entropy || out.mutual || out.counts) {
        const float h = entropy_of<KK>(mean, K);
        if (out.entropy) out.entropy[px] = h;
        if (out.mutual) out.mutual[px] = fmaxf(h - hs[p] / tf, 0.f);
        const float sc = h * H_SCALE;
        if (fabsf(sc) < 2147483648.f) hq[p] = (int)rintf(sc);                  // (false for a NaN or an infinity: never converted)
      }
      if (out.votes) {
        unsigned v = 0;
#pragma unroll
        for (int t = 0; t < MAXT; ++t)
          if (t < T) v += label_at(lab[p], t) == arg;
        out.votes[px] = (uint8_t)v;
      }
    }
  }
  if (!out.counts) return;                                   // (uniform)

  // ---- counts: wave votes per class that occurs in the wave
  const int lane = threadIdx.x & 63;
  unsigned mine = 0;
#pragma unroll
  for (int p = 0; p < PPL; ++p)
    if (valid[p]) mine |= seen[p] | (1u << pr[p]);
  unsigned present = 0;
  for (int k = 0; k < K; ++k)
    if (__ballot((mine >> k) & 1u)) present |= 1u << k;
  present = __builtin_amdgcn_readfirstlane(present);
  for (int k = 0; k < K; ++k) {
    if (!((present >> k) & 1u)) continue;                    // (wave-uniform)
    int mine = 0;                                            // lane i: the wave's count for slot i of row k
    unsigned v = 0, all = 0, any = 0;
    int hv = 0;
    unsigned long long is_k[PPL];                            // the lanes whose pixel p is predicted k
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
      const bool ip = valid[p] && pr[p] == (unsigned)k;
      is_k[p] = __ballot(ip);
      v += __popcll(is_k[p]);
      all += __popcll(__ballot(valid[p] && seen[p] == (1u << k)));
      any += __popcll(__ballot(valid[p] && ((seen[p] >> k) & 1u)));
      hv += ip ? hq[p] : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) hv += __shfl_xor(hv, o, 64);               // |hv| < 2^31: 256 pixels of at most ln 32 * 2^20
    mine = lane == SLOT_V ? (int)v : lane == SLOT_ALL ? (int)all : lane == SLOT_ANY ? (int)any : lane == SLOT_HSUM ? hv : 0;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      if (t < T) {                                           // (uniform)
        unsigned vt = 0, it = 0;
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
          const unsigned long long at = __ballot(valid[p] && label_at(lab[p], t) == (unsigned)k);
          vt += __popcll(at);
          it += __popcll(at & is_k[p]);
        }
        mine = lane == SLOT_VT + t ? (int)vt : lane == SLOT_VT + T + t ? (int)it : mine;
      }
    }
    // (a count is below 2^31 and HSUM's share may be negative: sign-extended, the two's complement sum subtracts)
    if (lane < slots && mine) atomicAdd(cnt + (size_t)k * slots + lane, (unsigned long long)(long long)mine);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * slots; i += TPB)
    if (cnt[i]) atomicAdd(out.counts + i, cnt[i]);
}

}  // namespace

extern "C" {

int smsut_tta_uncertain(const float* const* members, const int* transforms, uint8_t* pred, float* conf, float* entropy, float* mutual,
                        uint8_t* votes, int64_t* counts, int T, int N, int H, int W, int C, int K, void* stream) {
  SMSUT_REQUIRE(T >= 1 && T <= MAXT && N >= 0 && N <= SMSUT_TTA_MAX_SLICES && H >= 1 && W >= 1 && H <= SMSUT_TTA_MAX_DIM &&
                W <= SMSUT_TTA_MAX_DIM && K >= 1 && K <= C && K <= MAXK);
  SMSUT_REQUIRE(members && transforms && tta_list_ok(transforms, T, H, W));
  if (N == 0) return SMSUT_OK;
  SMSUT_REQUIRE(pred && ((uintptr_t)counts & 7) == 0);
  TtaMembers mem = {};
  for (int t = 0; t < T; ++t) {
    SMSUT_REQUIRE(members[t] && ((uintptr_t)members[t] & 3) == 0);
    mem.z[t] = members[t];
    mem.g[t] = (unsigned char)transforms[t];
  }
  const UncertainOut out = {pred, conf, entropy, mutual, votes, (unsigned long long*)counts};
  const TtaTiling tl = tta_tiling(C, K);
  const bool staged = tl.staged, big = tl.big;
  const dim3 grid((unsigned)((W + tl.ts - 1) / tl.ts), (unsigned)((H + tl.ts - 1) / tl.ts), (unsigned)N);
  // the staged tile (rounded up to 8 bytes), then the workgroup's counters: at most 33856 + 32 * 36 * 8 = 43072 bytes
  const int tile_floats = (int)((tl.tile_bytes / sizeof(float) + 1) & ~(size_t)1);
  const size_t lds = (size_t)tile_floats * sizeof(float) + (counts ? (size_t)K * (2 * T + SLOT_VT) * sizeof(unsigned long long) : 0);
#define UNC_L(KT, PPL, ST) k_tta_uncertain<KT, PPL, ST><<<grid, TPB, lds, (hipStream_t)stream>>>(mem, out, T, H, W, C, K, tile_floats)
#define UNC_K(KT) do { if (big) UNC_L(KT, 4, true); else if (staged) UNC_L(KT, 1, true); else UNC_L(KT, 1, false); } while (0)
  switch (K) { case 2: UNC_K(2); break; case 3: UNC_K(3); break; case 4: UNC_K(4); break; case 5: UNC_K(5); break;
               default: if (staged) UNC_L(0, 1, true); else UNC_L(0, 1, false); }
#undef UNC_K
#undef UNC_L
  SMSUT_LAUNCH_CHECK(); return SMSUT_OK;
}

}  // extern "C"
