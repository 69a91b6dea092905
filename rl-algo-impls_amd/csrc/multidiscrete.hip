// MultiDiscrete actor head (flat, non-GridNet factored action spaces) and flat action masks for gfx950.
//
// Reference regions replaced:
//   rl_algo_impls/shared/actor/multi_discrete.py:15-66   MultiCategorical (log_prob, entropy, sample)
//   rl_algo_impls/shared/actor/multi_discrete.py:69-105  MultiDiscreteActorHead.forward (final Linear + pi_forward)
//   rl_algo_impls/shared/actor/categorical.py:12-54      MaskedCategorical (masked logits, masked entropy)
//
// Shapes are small (H <= 512, A = sum(nvec) <= 256, G <= 32, B a few dozen to a few thousand), so the layout
// serves few, short launches: one wave64 per row for the forward, the sampler and the backward's row pass
// (lane layout and the shared row arithmetic in md_row.h); the weight gradient is one thread per (a, h)
// walking the batch upwards (a fixed-order reduction: no atomics, two calls give the same bits).
#include "md_row.h"

namespace {

constexpr int ROWS_PER_BLOCK = 4;  // one wave per row, 256 threads

// logits[b, a] = x[b] . W[a] + bias[a] (double accumulation, rounded once), then logp / entropy of the row
// from the ROUNDED logits (what the backward and the sampler see).  actions == nullptr: logits only.
__global__ __launch_bounds__(256) void md_head_fwd_kernel(
    const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
    const uint8_t* __restrict__ mask, const int64_t* __restrict__ actions, int64_t B, int H, MdGroups gr,
    float* __restrict__ logits, float* __restrict__ logp, float* __restrict__ entropy) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  const bool live = row < B;
  const int64_t r = live ? row : B - 1;  // spare waves repeat the last row and store nothing
  const int A = gr.A;
  const float* xr = x + r * H;
  const float* wr[MD_K];
  double acc[MD_K];
#pragma unroll
  for (int k = 0; k < MD_K; ++k) {
    const int a = lane + 64 * k;
    wr[k] = W + (int64_t)(a < A ? a : A - 1) * H;
    acc[k] = 0.0;
  }
#pragma unroll 4
  for (int h = 0; h < H; ++h) {
    const double xv = (double)xr[h];
#pragma unroll
    for (int k = 0; k < MD_K; ++k) acc[k] += xv * (double)wr[k][h];
  }
  float z[MD_K];
  bool ok[MD_K];
#pragma unroll
  for (int k = 0; k < MD_K; ++k) {
    const int a = lane + 64 * k;
    const bool in = a < A;
    z[k] = in ? (float)(acc[k] + (double)bias[a]) : 0.f;
    ok[k] = in && (!mask || mask[r * A + a] != 0);
    if (in && live) logits[row * A + a] = z[k];
  }
  if (!actions) return;
  double lp = 0.0, en = 0.0, e[MD_K] = {0.0, 0.0, 0.0, 0.0};
  bool bad = false;
  for (int g = 0; g < gr.G; ++g) {
    const int lo = gr.off[g], hi = gr.off[g + 1];
    const MdGroupStats st = md_group_stats(z, ok, lane, lo, hi, e);
    const int tgt = md_target(actions[r * gr.G + g], lo, hi);
    bad = bad || tgt < 0;
    lp += md_group_logp(z, ok, lane, lo, hi, tgt, st);
    en += md_group_entropy(st);
  }
  if (live && lane == 0) {
    logp[row] = bad ? __builtin_nanf("") : (float)lp;  // an action outside its group: NaN, nothing is read
    entropy[row] = (float)en;
  }
}

// Backward, row pass.  Per group with lse its log-sum-exp, p = softmax, n = z - lse, Hg its entropy:
//   d_logits[a] = d_logp (1[a == action] - p[a]) - d_entropy p[a] (n[a] + Hg)      (valid a; 0 when masked
//   or in an all-false group), stored for the weight pass, and dx[b] = d_logits[b] . W.
__global__ __launch_bounds__(256) void md_head_bwd_rows_kernel(
    const float* __restrict__ W, const float* __restrict__ logits, const uint8_t* __restrict__ mask,
    const int64_t* __restrict__ actions, const float* __restrict__ d_logp, const float* __restrict__ d_entropy,
    int64_t B, int H, MdGroups gr, float* __restrict__ d_logits, float* __restrict__ dx) {
  __shared__ float dq_s[ROWS_PER_BLOCK][MD_MAX_A];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + w;
  const bool live = row < B;
  const int64_t r = live ? row : B - 1;
  const int A = gr.A;
  float z[MD_K];
  bool ok[MD_K];
  md_load_row(logits + r * A, mask ? mask + r * A : nullptr, A, lane, z, ok);
  const double gl = (double)d_logp[r], ge = (double)d_entropy[r];
  double e[MD_K] = {0.0, 0.0, 0.0, 0.0};
  float dq[MD_K] = {0.f, 0.f, 0.f, 0.f};
  for (int g = 0; g < gr.G; ++g) {
    const int lo = gr.off[g], hi = gr.off[g + 1];
    const MdGroupStats st = md_group_stats(z, ok, lane, lo, hi, e);
    if (!st.any) continue;  // uniform over the wave
    const int tgt = md_target(actions[r * gr.G + g], lo, hi);
    const double lse = (double)st.m + log(st.s0), Hg = md_group_entropy(st), inv = 1.0 / st.s0;
#pragma unroll
    for (int k = 0; k < MD_K; ++k) {
      const int a = lane + 64 * k;
      if (a >= lo && a < hi && ok[k]) {
        const double p = e[k] * inv, n = (double)z[k] - lse;
        dq[k] = (float)(gl * ((a == tgt ? 1.0 : 0.0) - p) - ge * p * (n + Hg));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < MD_K; ++k) {
    const int a = lane + 64 * k;
    if (a < A) {
      dq_s[w][a] = dq[k];
      if (live) d_logits[row * A + a] = dq[k];
    }
  }
  __syncthreads();
  constexpr int NJ = MD_MAX_H / 64;
  double acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.0;
  for (int a = 0; a < A; ++a) {
    const double q = (double)dq_s[w][a];
    const float* wa = W + (int64_t)a * H;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int h = lane + 64 * j;
      if (h < H) acc[j] += q * (double)wa[h];
    }
  }
  if (live) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int h = lane + 64 * j;
      if (h < H) dx[row * H + h] = (float)acc[j];
    }
  }
}

// Backward, weight pass: thread (a, h) sums d_logits[b, a] x[b, h] over b = 0, 1, ... (double, rounded once);
// the workgroups of the first h tile also sum the bias gradient.  Written, or added (accumulate).
__global__ __launch_bounds__(256) void md_head_bwd_weights_kernel(
    const float* __restrict__ x, const float* __restrict__ d_logits, int64_t B, int H, int A,
    float* __restrict__ dW, float* __restrict__ db, int accumulate) {
  const int lane = threadIdx.x & 63;
  const int a = (int)blockIdx.y * ROWS_PER_BLOCK + (threadIdx.x >> 6);
  const int h = (int)blockIdx.x * 64 + lane;
  if (a >= A) return;
  const int hc = h < H ? h : H - 1;
  double acc = 0.0, accb = 0.0;
#pragma unroll 8
  for (int64_t b = 0; b < B; ++b) {
    const double q = (double)d_logits[b * A + a];
    acc += q * (double)x[b * H + hc];
    accb += q;
  }
  if (h < H) {
    float* dst = dW + (int64_t)a * H + h;
    *dst = accumulate ? *dst + (float)acc : (float)acc;
  }
  if (blockIdx.x == 0 && lane == 0) db[a] = accumulate ? db[a] + (float)accb : (float)accb;
}

// Row n of an env step: per group an inverse-CDF draw over the VALID entries only (a masked entry adds no
// mass and is never compared), its log-prob through md_row.h from the stored action, the value pass-through.
// Group g draws u from Philox4x32-10 with key seed, counter (offset, 8 n + g / 4), word g % 4.  A group
// whose mask is all false has the reference's uniform distribution over its entries.
__global__ __launch_bounds__(256) void md_sample_kernel(
    const float* __restrict__ logits, const uint8_t* __restrict__ mask, int64_t N, MdGroups gr, uint64_t seed,
    uint64_t offset, int64_t* __restrict__ actions, float* __restrict__ logp, const float* __restrict__ v_in,
    float* __restrict__ v_out, int K) {
  __shared__ double es[ROWS_PER_BLOCK][MD_MAX_A];
  __shared__ uint8_t oks[ROWS_PER_BLOCK][MD_MAX_A];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * ROWS_PER_BLOCK + w;
  const bool live = row < N;
  const int64_t r = live ? row : N - 1;
  const int A = gr.A, G = gr.G;
  float z[MD_K];
  bool ok[MD_K];
  md_load_row(logits + r * A, mask ? mask + r * A : nullptr, A, lane, z, ok);
  double e[MD_K] = {0.0, 0.0, 0.0, 0.0};
  double my_s0 = 1.0;
  float my_m = 0.f;
  int my_any = 0;
  for (int g = 0; g < G; ++g) {
    const MdGroupStats st = md_group_stats(z, ok, lane, gr.off[g], gr.off[g + 1], e);
    if (lane == g) {
      my_s0 = st.s0;
      my_m = st.m;
      my_any = st.any ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < MD_K; ++k) {
    const int a = lane + 64 * k;
    if (a < A) {
      es[w][a] = e[k];
      oks[w][a] = ok[k] ? 1 : 0;
    }
  }
  __syncthreads();
  int act = 0;
  if (lane < G) {
    const int lo = gr.off[lane], hi = gr.off[lane + 1], n = hi - lo;
    const Philox4 rnd = philox4x32_10(offset, ((uint64_t)r << 3) | (uint64_t)(lane >> 2), seed);
    const uint32_t words[4] = {rnd.x, rnd.y, rnd.z, rnd.w};
    uint32_t word = words[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) word = (lane & 3) == q ? words[q] : word;
    const float u = u01_open0(word);  // (0, 1]
    if (!my_any) {
      act = (int)ceilf(u * (float)n) - 1;
      act = act < 0 ? 0 : (act > n - 1 ? n - 1 : act);
    } else {
      const double t = (double)u * my_s0;
      double c = 0.0;
      int last = 0;
      act = -1;
      for (int i = lo; i < hi; ++i) {
        if (!oks[w][i]) continue;
        last = i - lo;
        c += es[w][i];
        if (act < 0 && t <= c) act = i - lo;
      }
      if (act < 0) act = last;  // t beyond the running sum's last rounding: the last valid entry
    }
    if (live) actions[row * G + lane] = act;
  }
  double lp = 0.0;
  for (int g = 0; g < G; ++g) {
    MdGroupStats st;
    st.m = __shfl(my_m, g, 64);
    st.s0 = __shfl(my_s0, g, 64);
    st.s1 = 0.0;
    st.any = __shfl(my_any, g, 64) != 0;
    const int lo = gr.off[g], hi = gr.off[g + 1];
    lp += md_group_logp(z, ok, lane, lo, hi, lo + __shfl(act, g, 64), st);
  }
  if (live && lane == 0) logp[row] = (float)lp;
  if (live && v_in && v_out && lane < K) v_out[row * K + lane] = v_in[row * K + lane];
}

// nvec (host) -> group offsets.  RAI_E_SHAPE for a malformed nvec, RAI_E_UNSUPPORTED beyond the limits.
int md_groups(const int32_t* nvec, int32_t G, int32_t H, MdGroups* out) {
  if (G < 1 || H < 1) return RAI_E_SHAPE;
  if (G > MD_MAX_G || H > MD_MAX_H) return RAI_E_UNSUPPORTED;
  if (!nvec) return RAI_E_NULLPTR;
  int64_t A = 0;
  out->G = G;
  out->off[0] = 0;
  for (int g = 0; g < G; ++g) {
    if (nvec[g] < 1) return RAI_E_SHAPE;
    A += nvec[g];
    if (A > MD_MAX_A) return RAI_E_UNSUPPORTED;
    out->off[g + 1] = (uint16_t)A;
  }
  out->A = (int)A;
  return RAI_OK;
}

}  // namespace

extern "C" int rai_md_head_fwd(const float* x, const float* W, const float* b, const uint8_t* mask,
                               const int64_t* actions, const int32_t* nvec, int32_t G, int64_t B, int32_t H,
                               float* logits, float* logp, float* entropy, void* stream) {
  if (B < 0) return RAI_E_SHAPE;
  MdGroups gr;
  const int rc = md_groups(nvec, G, H, &gr);
  if (rc != RAI_OK) return rc;
  if (B == 0) return RAI_OK;
  if (!x || !W || !b || !logits || (actions && (!logp || !entropy))) return RAI_E_NULLPTR;
  const int64_t blocks = (B + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (blocks > 0x7fffffffLL) return RAI_E_SHAPE;
  hipLaunchKernelGGL(md_head_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, rai_stream(stream), x, W, b, mask,
                     actions, B, H, gr, logits, logp, entropy);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_md_head_bwd(const float* x, const float* W, const float* logits, const uint8_t* mask,
                               const int64_t* actions, const int32_t* nvec, int32_t G, const float* d_logp,
                               const float* d_entropy, int64_t B, int32_t H, float* d_logits, float* dx, float* dW,
                               float* db, int32_t accumulate, void* stream) {
  if (B < 0) return RAI_E_SHAPE;
  MdGroups gr;
  const int rc = md_groups(nvec, G, H, &gr);
  if (rc != RAI_OK) return rc;
  if (!dW || !db) return RAI_E_NULLPTR;
  if (B > 0 && (!x || !W || !logits || !actions || !d_logp || !d_entropy || !d_logits || !dx)) return RAI_E_NULLPTR;
  const int64_t blocks = (B + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (blocks > 0x7fffffffLL) return RAI_E_SHAPE;
  hipStream_t st = rai_stream(stream);
  if (B > 0) {
    hipLaunchKernelGGL(md_head_bwd_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, st, W, logits, mask, actions,
                       d_logp, d_entropy, B, H, gr, d_logits, dx);
    RAI_LAUNCH_CHECK();
  }
  // B == 0: the sums are empty, so the weight pass writes zeros (or adds nothing)
  const dim3 grid((unsigned)((H + 63) / 64), (unsigned)((gr.A + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK));
  hipLaunchKernelGGL(md_head_bwd_weights_kernel, grid, dim3(256), 0, st, x, d_logits, B, H, gr.A, dW, db,
                     accumulate ? 1 : 0);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_md_sample(const float* logits, const uint8_t* mask, const int32_t* nvec, int32_t G, int64_t N,
                             uint64_t seed, uint64_t offset, int64_t* actions_out, float* logp_out,
                             const float* v_in, float* v_out, int32_t K, void* stream) {
  if (N < 0 || K < 0 || K > 64) return RAI_E_SHAPE;
  MdGroups gr;
  const int rc = md_groups(nvec, G, 1, &gr);
  if (rc != RAI_OK) return rc;
  if (N == 0) return RAI_OK;
  if (!logits || !actions_out || !logp_out) return RAI_E_NULLPTR;
  const int64_t blocks = (N + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
  if (blocks > 0x7fffffffLL) return RAI_E_SHAPE;
  hipLaunchKernelGGL(md_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, rai_stream(stream), logits, mask, N, gr,
                     seed, offset, actions_out, logp_out, v_in, v_out, K);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}
