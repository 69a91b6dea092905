// One row of the gSDE actor head (rl_algo_impls/shared/actor/state_dependent_noise.py:35-78,140-154),
// shared by the head forward and the rollout's sample kernel (csrc/sde.hip): both go from the STORED
// action through the same functions below, so the log-probability the rollout logs and the one the
// first update pass recomputes are the same bits (PPO ratio exactly 1).
//
// Lane layout of one wave64 per row: AP = the power of two >= A (A <= 32, so AP <= 32 divides 64),
// action a = lane % AP, hidden group hg = lane / AP of G = 64 / AP groups; group hg walks
// h = hg, hg + G, ...  The (H, A) matrices (log_std, an exploration matrix) are read with a fastest, so
// consecutive lanes read consecutive addresses; latent[h] is a broadcast within a group.  The sums
// over h finish with log2(G) xor-shuffles across groups, the sums over a with log2(AP) inside a group:
// every lane ends with the same bits (each step adds two commuted operands), in a fixed order.
// Sums and the row's transcendental terms are carried in double and rounded once on store: the head is
// B x A elements of arithmetic, far from any throughput limit, and the f32 results are then within
// half an ulp of the formula instead of carrying the f32 libm's and a sequential sum's rounding.
#pragma once
#include "common.h"

constexpr float SDE_F32_EPS = 1.1920928955078125e-07f;  // torch.finfo(float32).eps (TanhBijector.inverse)
constexpr double SDE_LOG_SQRT_2PI = 0.91893853320467274178;

struct SdeLanes {
  int AP, shift;  // AP = 1 << shift
};
__host__ __device__ inline SdeLanes sde_lanes(int A) {
  SdeLanes l{1, 0};
  while (l.AP < A) {
    l.AP <<= 1;
    ++l.shift;
  }
  return l;
}

// sum over the hidden groups (lanes with the same a); all 64 lanes must be active
__device__ __forceinline__ double sde_sum_groups(double v, int AP) {
  for (int o = 32; o >= AP; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the AP action lanes of a group; all 64 lanes must be active
__device__ __forceinline__ double sde_sum_actions(double v, int AP) {
  for (int o = AP >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double sde_std(const float* __restrict__ log_std, int h, int a, int A, int full_std) {
  return exp((double)log_std[full_std ? h * A + a : h]);
}

// sigma[a] = sqrt(sum_h latent[h]^2 S[h, a]^2 + 1e-6) of one row, on every lane with that a
__device__ __forceinline__ double sde_row_sigma(const float* __restrict__ latent_row,
                                                const float* __restrict__ log_std, int H, int A, SdeLanes ln,
                                                int full_std, int lane) {
  const int a = lane & (ln.AP - 1), hg = lane >> ln.shift, G = 64 >> ln.shift;
  double acc = 0.0;
  if (a < A) {
    for (int h = hg; h < H; h += G) {
      const double l = (double)latent_row[h];
      const double s = sde_std(log_std, h, a, A, full_std);
      acc += (l * l) * (s * s);
    }
  }
  acc = sde_sum_groups(acc, ln.AP);
  return sqrt(acc + 1e-6);
}

// the Gaussian-space action: a itself, or atanh(clamp(a, -1 + eps, 1 - eps)) when squashing
__device__ __forceinline__ double sde_gaussian_action(float act, int squash) {
  if (!squash) return (double)act;
  const float c = fminf(fmaxf(act, -1.f + SDE_F32_EPS), 1.f - SDE_F32_EPS);
  return atanh((double)c);
}

// log-probability and entropy of one row from its stored action: this lane's action term (lanes with
// a >= A add nothing), summed over the group's action lanes.  squash: the tanh correction
// sum_a log(1 - tanh(g)^2 + 1e-6) is subtracted and the entropy is -logp (pi_forward).
__device__ __forceinline__ void sde_row_logp_entropy(float act, float mu, double sigma, bool valid, int squash,
                                                     int AP, float* logp, float* entropy) {
  double lp = 0.0, en = 0.0;
  if (valid) {
    const double g = sde_gaussian_action(act, squash);
    const double d = g - (double)mu;
    const double log_sigma = log(sigma);
    lp = -(d * d) / (2.0 * sigma * sigma) - log_sigma - SDE_LOG_SQRT_2PI;
    if (squash) {
      const double t = tanh(g);
      lp -= log(1.0 - t * t + 1e-6);
    }
    en = 0.5 + SDE_LOG_SQRT_2PI + log_sigma;
  }
  lp = sde_sum_actions(lp, AP);
  en = sde_sum_actions(en, AP);
  *logp = (float)lp;
  *entropy = squash ? -(float)lp : (float)en;
}
