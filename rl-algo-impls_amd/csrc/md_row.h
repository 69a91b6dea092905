// One row of the MultiDiscrete actor head (rl_algo_impls/shared/actor/multi_discrete.py MultiCategorical over
// rl_algo_impls/shared/actor/categorical.py MaskedCategorical), shared by the head forward, its backward and
// the rollout's sample kernel (csrc/multidiscrete.hip): all three go from the row's float32 logits through
// the functions below, so the log-probability the rollout logs and the one the first update pass recomputes
// are the same bits (PPO ratio exactly 1).
//
// Lane layout of one wave64 per row: logit a = lane + 64 k, k < 4 (A <= 256), so a row's logits, masks and
// gradients are coalesced and live in four registers per lane.  A group g is the contiguous run
// [off[g], off[g + 1]) of a; its sums are whole-wave reductions in which lanes outside the group add zero
// (one float max through __shfl_xor, the sums by DPP, common.h), so every lane ends with the same bits in a
// fixed order.  Sums and transcendentals are carried in double and rounded once on store.
//
// Masked logits are finfo(float32).min (MaskedCategorical); a group's logits are normalised by its own
// log-sum-exp.  A group whose mask is all false: in float32 finfo.min + log n rounds back to finfo.min, so
// the reference's normalised logits are 0 there: log-prob 0, (masked) entropy 0, no gradient.
#pragma once
#include "common.h"

constexpr int MD_MAX_H = RAI_MD_MAX_H, MD_MAX_A = RAI_GRID_MAX_A, MD_MAX_G = RAI_MD_MAX_G;
constexpr int MD_K = MD_MAX_A / 64;  // logits per lane

struct MdGroups {
  int G, A;
  uint16_t off[MD_MAX_G + 1];  // off[0] = 0, off[G] = A
};

struct MdGroupStats {
  float m;     // max of the group's (masked) logits
  double s0;   // sum_i exp(x_i - m) over the valid entries
  double s1;   // sum_i exp(x_i - m) (x_i - m)
  bool any;    // some entry is valid
};

// This lane's logits of one row: z[k] and ok[k] (inside the row and not masked) for a = lane + 64 k.
__device__ __forceinline__ void md_load_row(const float* __restrict__ zrow, const uint8_t* __restrict__ mrow, int A,
                                            int lane, float (&z)[MD_K], bool (&ok)[MD_K]) {
#pragma unroll
  for (int k = 0; k < MD_K; ++k) {
    const int a = lane + 64 * k;
    const bool in = a < A;
    z[k] = in ? zrow[a] : 0.f;
    ok[k] = in && (!mrow || mrow[a] != 0);
  }
}

// Group [lo, hi): its statistics on every lane, and e[k] = exp(z[k] - m) for this lane's valid entries of
// the group (entries of other groups are left alone).  All 64 lanes must be active.
__device__ __forceinline__ MdGroupStats md_group_stats(const float (&z)[MD_K], const bool (&ok)[MD_K], int lane,
                                                       int lo, int hi, double (&e)[MD_K]) {
  MdGroupStats st;
  float m = -INFINITY;
  bool any = false;
#pragma unroll
  for (int k = 0; k < MD_K; ++k) {
    const int a = lane + 64 * k;
    if (a >= lo && a < hi) {
      m = fmaxf(m, ok[k] ? z[k] : RAI_F32_MIN);
      any = any || ok[k];
    }
  }
  st.m = wave_max(m);
  st.any = __ballot(any) != 0ULL;
  double s0 = 0.0, s1 = 0.0;
#pragma unroll
  for (int k = 0; k < MD_K; ++k) {
    const int a = lane + 64 * k;
    if (a >= lo && a < hi) {
      const double d = (double)z[k] - (double)st.m;
      e[k] = ok[k] ? exp(d) : 0.0;
      s0 += e[k];
      s1 += e[k] * d;
    }
  }
  st.s0 = wave_sum_dpp(s0);
  st.s1 = wave_sum_dpp(s1);
  return st;
}

// log-prob of entry `target` (an index into the row; outside [lo, hi) selects nothing) under the group's
// distribution.  The selection is a wave sum with one non-zero term, so it is exact.
__device__ __forceinline__ double md_group_logp(const float (&z)[MD_K], const bool (&ok)[MD_K], int lane, int lo,
                                                int hi, int target, const MdGroupStats& st) {
  float x = 0.f;
#pragma unroll
  for (int k = 0; k < MD_K; ++k) {
    const int a = lane + 64 * k;
    if (a >= lo && a < hi && a == target) x = ok[k] ? z[k] : RAI_F32_MIN;
  }
  x = wave_sum_dpp(x);
  if (!st.any) return 0.0;
  return (double)x - ((double)st.m + log(st.s0));
}

// entropy of the group: -sum_valid p log p = log s0 - s1 / s0 (the masked and the plain form agree: a
// masked entry has p = 0)
__device__ __forceinline__ double md_group_entropy(const MdGroupStats& st) {
  return st.any ? log(st.s0) - st.s1 / st.s0 : 0.0;
}

// Action g of a row as an index into the row, or -1 when it is outside its group
__device__ __forceinline__ int md_target(int64_t act, int lo, int hi) {
  return act >= 0 && act < (int64_t)(hi - lo) ? lo + (int)act : -1;
}
