// gSDE (generalised state-dependent exploration) actor head for gfx950.
//
// Reference regions replaced:
//   rl_algo_impls/shared/actor/state_dependent_noise.py:35-78   StateDependentNoiseDistribution
//                                                               (log_prob, sample, _get_noise)
//   rl_algo_impls/shared/actor/state_dependent_noise.py:140-163 _distribution: variance, sigma
//   rl_algo_impls/shared/actor/state_dependent_noise.py:177-182 sample_weights
//   rl_algo_impls/shared/actor/state_dependent_noise.py:189-199 pi_forward (entropy)
//   rl_algo_impls/shared/policy/actor_critic.py:62-87           clamp_actions
//
// Shapes are tiny (H <= 512, A <= 32, B a few dozen to a few thousand), so the layout serves few,
// short launches rather than throughput: one wave64 per row for the forward and the sample (lane
// layout in sde_row.h, no LDS), and for the log_std gradient one thread per (h, a) walking the batch
// in ascending order (a fixed-order reduction, no atomics, no workspace, one launch).
#include "sde_row.h"

namespace {

constexpr int ROWS_PER_BLOCK = 4;  // one wave per row, 256 threads

__global__ __launch_bounds__(256) void sde_head_fwd_kernel(
    const float* __restrict__ latent, const float* __restrict__ mu, const float* __restrict__ log_std,
    const float* __restrict__ actions, int64_t B, int H, int A, SdeLanes ln, int full_std, int squash,
    float* __restrict__ logp, float* __restrict__ entropy, float* __restrict__ sigma) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (b >= B) return;  // whole waves leave together
  const int a = lane & (ln.AP - 1);
  const bool valid = a < A;
  const double sg = sde_row_sigma(latent + b * H, log_std, H, A, ln, full_std, lane);
  float act = 0.f, m = 0.f;
  if (valid) {
    act = actions[b * A + a];
    m = mu[b * A + a];
    if (lane < ln.AP) sigma[b * A + a] = (float)sg;
  }
  float lp, en;
  sde_row_logp_entropy(act, m, sg, valid, squash, ln.AP, &lp, &en);
  if (lane == 0) {
    logp[b] = lp;
    entropy[b] = en;
  }
}

// d_mu and d_log_std.  With g the Gaussian-space action, d = g - mu and (squash: entropy = -logp)
// gl = d_logp - d_entropy, ge = 0; else gl = d_logp, ge = d_entropy:
//   d_mu[b, a]    = gl d / sigma^2
//   d_sigma[b, a] = gl (d^2 / sigma^3 - 1 / sigma) + ge / sigma,   d_var = d_sigma / (2 sigma)
//   d_log_std[h, a] = sum_b d_var[b, a] latent[b, h]^2 2 S[h, a]^2   (summed over a too when not full_std)
// Thread (hl, a) of a workgroup owns h = blockIdx.x * HB + hl (HB = 256 / AP) and walks b upwards in chunks
// of HB rows: per chunk, thread (r, a) computes d_var of row b0 + r into LDS (workgroup 0 also stores d_mu),
// then every thread adds its HB products.  The tanh correction depends on the action alone: no gradient.
__global__ __launch_bounds__(256) void sde_head_bwd_kernel(
    const float* __restrict__ latent, const float* __restrict__ mu, const float* __restrict__ log_std,
    const float* __restrict__ actions, const float* __restrict__ sigma, const float* __restrict__ d_logp,
    const float* __restrict__ d_entropy, int64_t B, int H, int A, SdeLanes ln, int full_std, int squash,
    float* __restrict__ d_mu, float* __restrict__ d_log_std, int accumulate) {
  __shared__ double dv[256];
  const int tid = threadIdx.x;
  const int a = tid & (ln.AP - 1), hl = tid >> ln.shift;
  const int HB = 256 >> ln.shift;
  const int h = (int)blockIdx.x * HB + hl;
  const bool live = a < A && h < H;
  double acc = 0.0;
  for (int64_t b0 = 0; b0 < B; b0 += HB) {
    const int64_t b = b0 + hl;
    double v = 0.0;
    if (b < B && a < A) {
      const int64_t i = b * A + a;
      const double sg = (double)sigma[i];
      const double d = sde_gaussian_action(actions[i], squash) - (double)mu[i];
      double gl = (double)d_logp[b], ge = (double)d_entropy[b];
      if (squash) {
        gl -= ge;
        ge = 0.0;
      }
      const double inv = 1.0 / sg;
      if (blockIdx.x == 0) d_mu[i] = (float)(gl * d * inv * inv);
      v = (gl * (d * d * inv * inv * inv - inv) + ge * inv) * 0.5 * inv;
    }
    __syncthreads();  // the previous chunk's readers are done with dv
    dv[tid] = v;
    __syncthreads();
    if (live) {
      const int nr = B - b0 < HB ? (int)(B - b0) : HB;
      const float* lrow = latent + b0 * H + h;
#pragma unroll 4
      for (int r = 0; r < nr; ++r) {
        const double l = (double)lrow[(int64_t)r * H];
        acc += dv[(r << ln.shift) | a] * (l * l);
      }
    }
  }
  double out = 0.0;
  if (live) {
    const double s = sde_std(log_std, h, a, A, full_std);
    out = acc * (2.0 * (s * s));
  }
  if (!full_std) out = sde_sum_actions(out, ln.AP);  // the group's AP lanes are one aligned run of a wave
  if (h < H && (full_std ? a < A : a == 0)) {
    const int i = full_std ? h * A + a : h;
    d_log_std[i] = accumulate ? d_log_std[i] + (float)out : (float)out;
  }
}

// E[n, h, a] = S[h, a] eps, n < N, and E0[h, a] (flat index n = N).  Thread q draws the four normals of flat
// elements 4q .. 4q + 3 from ONE Philox4x32-10 block, key seed, counter (offset, q): no two elements share a
// draw, and (seed, offset) fixes every element.  Box-Muller as gaussian_sample_kernel (rollout.hip).
__global__ __launch_bounds__(256) void sde_sample_weights_kernel(const float* __restrict__ log_std, int64_t N,
                                                                 int H, int A, int full_std, uint64_t seed,
                                                                 uint64_t offset, float* __restrict__ E,
                                                                 float* __restrict__ E0) {
  const int64_t HA = (int64_t)H * A;
  const int64_t total = (N + 1) * HA;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (4 * q >= total) return;
  const Philox4 rnd = philox4x32_10(offset, (uint64_t)q, seed);
  const uint32_t u[4] = {rnd.x, rnd.y, rnd.z, rnd.w};
  float e[4];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = u01_open0(u[2 * p]), u2 = u01_open0(u[2 * p + 1]);
    const float rad = sqrtf(-2.f * logf(u1));
    float s, c;
    sincosf(6.283185307179586f * u2, &s, &c);
    e[2 * p] = rad * c;
    e[2 * p + 1] = rad * s;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = 4 * q + k;
    if (i >= total) break;
    const int64_t j = i % HA;
    const int h = (int)(j / A), a = (int)(j - (int64_t)h * A);
    const float v = (float)(sde_std(log_std, h, a, A, full_std) * (double)e[k]);
    if (i < N * HA) E[i] = v;
    else E0[j] = v;
  }
}

// Row n: x = mu[n] + latent[n] . E[n] (e_stride == 0: the one shared matrix), a = tanh(x) when squashing;
// the clamped action (clip to the bounds, or low + 0.5 (a + 1) (high - low) when squashing); logp of the
// STORED a through sde_row.h; the value pass-through.
__global__ __launch_bounds__(256) void sde_sample_kernel(
    const float* __restrict__ mu, const float* __restrict__ latent, const float* __restrict__ log_std,
    const float* __restrict__ E, int64_t e_stride, int64_t N, int H, int A, SdeLanes ln, int full_std, int squash,
    const float* __restrict__ low, const float* __restrict__ high, float* __restrict__ actions,
    float* __restrict__ clamped, float* __restrict__ logp, const float* __restrict__ v_in,
    float* __restrict__ v_out, int K) {
  const int lane = threadIdx.x & 63;
  const int64_t n = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  if (n >= N) return;
  const int a = lane & (ln.AP - 1), hg = lane >> ln.shift, G = 64 >> ln.shift;
  const bool valid = a < A;
  const float* lrow = latent + n * H;
  const double sg = sde_row_sigma(lrow, log_std, H, A, ln, full_std, lane);
  const float* En = E + n * e_stride;
  double noise = 0.0;
  if (valid)
    for (int h = hg; h < H; h += G) noise += (double)lrow[h] * (double)En[h * A + a];
  noise = sde_sum_groups(noise, ln.AP);
  float act = 0.f, m = 0.f;
  if (valid) {
    m = mu[n * A + a];
    const double x = (double)m + noise;
    act = squash ? (float)tanh(x) : (float)x;
    if (lane < ln.AP) {
      actions[n * A + a] = act;
      if (clamped) {
        float c = act;
        if (squash) {
          c = low[a] + 0.5f * (act + 1.f) * (high[a] - low[a]);
        } else {
          if (low) c = fmaxf(c, low[a]);
          if (high) c = fminf(c, high[a]);
        }
        clamped[n * A + a] = c;
      }
    }
  }
  float lp, en;
  sde_row_logp_entropy(act, m, sg, valid, squash, ln.AP, &lp, &en);
  if (lane == 0) logp[n] = lp;
  if (v_in && v_out && lane < K) v_out[n * K + lane] = v_in[n * K + lane];
}

bool sde_in_limits(int32_t H, int32_t A) { return H >= 1 && H <= RAI_SDE_MAX_H && A >= 1 && A <= RAI_SDE_MAX_A; }

}  // namespace

extern "C" int rai_sde_head_fwd(const float* latent, const float* mu, const float* log_std, const float* actions,
                                int64_t B, int32_t H, int32_t A, int32_t full_std, int32_t squash, float* logp,
                                float* entropy, float* sigma, void* stream) {
  if (B < 0 || H < 1 || A < 1) return RAI_E_SHAPE;
  if (!sde_in_limits(H, A)) return RAI_E_UNSUPPORTED;
  if (B == 0) return RAI_OK;
  if (!latent || !mu || !log_std || !actions || !logp || !entropy || !sigma) return RAI_E_NULLPTR;
  const int64_t blocks = (B + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (blocks > 0x7fffffffLL) return RAI_E_SHAPE;
  hipLaunchKernelGGL(sde_head_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, rai_stream(stream), latent, mu,
                     log_std, actions, B, H, A, sde_lanes(A), full_std ? 1 : 0, squash ? 1 : 0, logp, entropy, sigma);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_sde_head_bwd(const float* latent, const float* mu, const float* log_std, const float* actions,
                                const float* sigma, const float* d_logp, const float* d_entropy, int64_t B, int32_t H,
                                int32_t A, int32_t full_std, int32_t squash, float* d_mu, float* d_log_std,
                                int32_t accumulate, void* stream) {
  if (B < 0 || H < 1 || A < 1) return RAI_E_SHAPE;
  if (!sde_in_limits(H, A)) return RAI_E_UNSUPPORTED;
  if (!log_std || !d_log_std) return RAI_E_NULLPTR;
  if (B > 0 && (!latent || !mu || !actions || !sigma || !d_logp || !d_entropy || !d_mu)) return RAI_E_NULLPTR;
  const SdeLanes ln = sde_lanes(A);
  const int HB = 256 >> ln.shift;
  hipLaunchKernelGGL(sde_head_bwd_kernel, dim3((unsigned)((H + HB - 1) / HB)), dim3(256), 0, rai_stream(stream),
                     latent, mu, log_std, actions, sigma, d_logp, d_entropy, B, H, A, ln, full_std ? 1 : 0,
                     squash ? 1 : 0, d_mu, d_log_std, accumulate ? 1 : 0);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_sde_sample_weights(const float* log_std, int64_t N, int32_t H, int32_t A, int32_t full_std,
                                      uint64_t seed, uint64_t offset, float* E, float* E0, void* stream) {
  if (N < 0 || H < 1 || A < 1) return RAI_E_SHAPE;
  if (!sde_in_limits(H, A)) return RAI_E_UNSUPPORTED;
  if (!log_std || !E0 || (N > 0 && !E)) return RAI_E_NULLPTR;
  const int64_t quads = ((N + 1) * (int64_t)H * A + 3) / 4;
  const int64_t blocks = (quads + 255) / 256;
  if (blocks > 0x7fffffffLL) return RAI_E_SHAPE;
  hipLaunchKernelGGL(sde_sample_weights_kernel, dim3((unsigned)blocks), dim3(256), 0, rai_stream(stream), log_std, N,
                     H, A, full_std ? 1 : 0, seed, offset, E, E0);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_sde_sample(const float* mu, const float* latent, const float* log_std, const float* E,
                              int64_t e_stride, int64_t N, int32_t H, int32_t A, int32_t full_std, int32_t squash,
                              const float* low, const float* high, float* actions_out, float* clamped_out,
                              float* logp_out, const float* v_in, float* v_out, int32_t K, void* stream) {
  if (N < 0 || H < 1 || A < 1 || K < 0 || K > 64 || e_stride < 0) return RAI_E_SHAPE;
  if (e_stride != 0 && e_stride < (int64_t)H * A) return RAI_E_SHAPE;
  if (!sde_in_limits(H, A)) return RAI_E_UNSUPPORTED;
  if (N == 0) return RAI_OK;
  if (!mu || !latent || !log_std || !E || !actions_out || !logp_out) return RAI_E_NULLPTR;
  if (squash && clamped_out && (!low || !high)) return RAI_E_NULLPTR;
  const int64_t blocks = (N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (blocks > 0x7fffffffLL) return RAI_E_SHAPE;
  hipLaunchKernelGGL(sde_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, rai_stream(stream), mu, latent, log_std,
                     E, e_stride, N, H, A, sde_lanes(A), full_std ? 1 : 0, squash ? 1 : 0, low, high, actions_out,
                     clamped_out, logp_out, v_in, v_out, K);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}
