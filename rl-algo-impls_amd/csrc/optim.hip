// Fused clip_grad_norm_ + Adam / RMSprop over one flat fp32 parameter buffer.
//
// Restates rl_algo_impls/ppo/ppo.py:441-447 (optimizer_step: clip_grad_norm_ ->
// Adam(eps=1e-7).step() -> zero_grad) with torch's update formulas
// (torch/optim/adam.py _single_tensor_adam / _multi_tensor_adam):
//   m   = lerp(m, g, 1-b1)            v = v*b2 + (1-b2)*g*g
//   denom = sqrt(v)/sqrt(1-b2^t) + eps
//   p  += -(lr/(1-b1^t)) * (m/denom)
// and rl_algo_impls/a2c/a2c.py:45-50,202-205 (RMSprop, alpha=0.99):
//   s = s*alpha + (1-alpha)*g*g ;  p += -lr * g/(sqrt(s)+eps)
// clip: total = ||g||_2 ; coef = max_norm/(total+1e-6) clamped to 1 ; g *= coef.
//
// Deterministic.  Two-launch form (any alignment / size):
//   K1 per-block partial sum of squares (fp64) -> workspace
//   K2 every block re-reduces the partials in the same fixed order (identical
//      result in every block), then scales, updates, and zeroes its slice.
// The step counter and grad-norm slot live in device memory (rai_train_state)
// so a captured graph replays correctly.
//
// Run-wise form (rai_clip_optim_step_runs; PPO's freeze_* options): the same two launches over a
// device table of runs [begin, end) that partition [0, P).  K1 sums the ACTIVE runs only
// (clip_grad_norm_ skips tensors without a gradient).  K2 updates each active run with its own
// bias corrections (Adam step = opt_step - lag: torch keeps state['step'] per tensor and
// Adam.step() skips a tensor without a gradient, so runs that sat out updates lag behind) and, for a
// frozen run, stores zeros to the gradient and touches nothing else.  The table is read-only on the
// device: the host rewrites it between updates, a captured graph replays unchanged.  One active
// run [0, P) with lag 0 walks exactly as the flat form does: bit-identical partials and outputs.
#include "common.h"
#include "internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_MAX_BLOCKS = 512;
constexpr int OPT_VEC = 4;

// ---- the pieces both forms (flat, run-wise) are made of -------------------------------------
// A span is [begin, end) of the flat buffer with a float4 interior [a0, a1) (16-byte aligned in
// every buffer the caller touches; a0 == a1 when there is none) and scalar ends [begin, a0) and
// [a1, end).  The flat kernels pass {0, 0, 4 * (P / 4) or 0, P}; the run-wise ones one span per run.
// Elements map to (block, thread) by their offset into the interior / the ends, so a single run
// [0, P) walks exactly as the flat form does.
struct OptSpan {
  int64_t begin, a0, a1, end;
};

__device__ __forceinline__ OptSpan run_span(int64_t begin, int64_t end, int vec) {
  OptSpan s = {begin, begin, begin, end};
  if (vec) {
    s.a0 = (begin + 3) & ~(int64_t)3;
    if (s.a0 > end) s.a0 = end;
    s.a1 = end & ~(int64_t)3;
    if (s.a1 < s.a0) s.a1 = s.a0;
  }
  return s;
}

// offset k into a span's scalar ends -> element index
__device__ __forceinline__ int64_t span_end_index(const OptSpan& sp, int64_t k) {
  const int64_t head = sp.a0 - sp.begin;
  return k < head ? sp.begin + k : sp.a1 + (k - head);
}

__device__ __forceinline__ double span_sumsq(const float* __restrict__ g, const OptSpan& sp, double s) {
  const int64_t stride = (int64_t)gridDim.x * OPT_THREADS;
  const int64_t gtid = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  const int64_t nvec = (sp.a1 - sp.a0) / OPT_VEC;
  const float4* g4 = reinterpret_cast<const float4*>(g + sp.a0);
  for (int64_t i = gtid; i < nvec; i += stride) {
    const float4 x = g4[i];
    s += (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
  }
  const int64_t nend = (sp.a0 - sp.begin) + (sp.end - sp.a1);
  for (int64_t k = gtid; k < nend; k += stride) {
    const int64_t i = span_end_index(sp, k);
    s += (double)g[i] * g[i];
  }
  return s;
}

// block partial -> workspace; block 0 advances the step: K2 (next in stream order) reads the new one
__device__ __forceinline__ void publish_partial(double s, double* partial, rai_train_state* state) {
  __shared__ double red[OPT_THREADS / 64];
  double v[1] = {s};
  block_sum<1>(v, red);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = v[0];
    if (blockIdx.x == 0) state->opt_step += 1;
  }
}

// identical fixed-order reduction of the partials in every block -> the clip coefficient; block 0
// records the pre-clip norm
__device__ __forceinline__ float clip_coef(const rai_optim_hparams& hp, rai_train_state* state,
                                           const double* __restrict__ partial, int nparts, float* norms,
                                           int max_norms) {
  __shared__ double red[OPT_THREADS / 64];
  double t = 0.0;
  for (int i = threadIdx.x; i < nparts; i += OPT_THREADS) t += partial[i];
  double v[1] = {t};
  block_sum<1>(v, red);
  const float total_norm = (float)sqrt(v[0]);
  float coef = 1.f;
  if (hp.max_grad_norm > 0.f) {
    coef = hp.max_grad_norm / (total_norm + 1e-6f);
    coef = fminf(coef, 1.f);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int ni = state->norm_index;
    if (norms && ni < max_norms) norms[ni] = total_norm;
    state->norm_index = ni + 1;
  }
  return coef;
}

// the constants of one optimizer step at step count `step` (per run in the run-wise form)
struct OptConsts {
  float c1, c2, c3, c4;  // Adam: w1, w2, bc2_sqrt, neg_step; RMSprop: w, neg_lr, -, -
};

__device__ __forceinline__ OptConsts opt_consts(const rai_optim_hparams& hp, int64_t step) {
  OptConsts c;
  if (hp.kind == 0) {
    const double bc1 = 1.0 - ipow(hp.beta1_d, step);
    const double bc2 = 1.0 - ipow(hp.beta2_d, step);
    c.c1 = (float)(1.0 - hp.beta1_d);   // lerp weight (torch: 1 - beta1 in Python)
    c.c2 = (float)(1.0 - hp.beta2_d);   // addcmul value
    c.c3 = (float)sqrt(bc2);
    c.c4 = (float)(-((double)hp.lr / bc1));
  } else {
    c.c1 = (float)(1.0 - hp.beta1_d);  // RMSprop: beta1_d carries alpha as a Python float
    c.c2 = -hp.lr;
    c.c3 = c.c4 = 0.f;
  }
  return c;
}

// the per-element update (torch's formulas, no contraction)
__device__ __forceinline__ void opt_update(const rai_optim_hparams& hp, const OptConsts& c, float coef,
                                           float graw, float& pp, float& m, float& vv) {
  const float gi = graw * coef;
  if (hp.kind == 0) {
    m = m + c.c1 * (gi - m);
    vv = vv * hp.beta2;
    vv = vv + (c.c2 * gi) * gi;
    const float denom = sqrtf(vv) / c.c3 + hp.eps;
    pp = pp + c.c4 * (m / denom);
  } else {
    float sq = m * hp.alpha;  // RMSprop keeps its square average in s1
    sq = sq + (c.c1 * gi) * gi;
    const float avg = sqrtf(sq) + hp.eps;
    pp = pp + c.c2 * (gi / avg);
    m = sq;
  }
}

// Update one span and zero its gradient (zero_grad).  float4 interior: two vectors per thread in
// flight per iteration (the scalar grid-stride loop was ~13 dependent round trips per thread at C3's
// 1.69M parameters: 12.8 us per step); then the scalar ends.  Same arithmetic per element, same results.
__device__ __forceinline__ void span_update(float* __restrict__ p, float* __restrict__ g,
                                            float* __restrict__ s1, float* __restrict__ s2,
                                            const OptSpan& sp, const rai_optim_hparams& hp,
                                            const OptConsts& c, float coef) {
  const bool adam = hp.kind == 0;
  const int64_t stride = (int64_t)gridDim.x * OPT_THREADS;
  const int64_t gtid = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  const int64_t nv = (sp.a1 - sp.a0) / OPT_VEC;
  float4* p4 = reinterpret_cast<float4*>(p + sp.a0);
  float4* g4 = reinterpret_cast<float4*>(g + sp.a0);
  float4* m4 = reinterpret_cast<float4*>(s1 + sp.a0);
  float4* v4 = reinterpret_cast<float4*>(s2 + sp.a0);
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t i = gtid; i < nv; i += 2 * stride) {
    const int64_t i2 = i + stride;
    const bool two = i2 < nv;
    float4 ga = g4[i], pa = p4[i], ma = m4[i], va = adam ? v4[i] : zero;
    float4 gb = zero, pb = zero, mb = zero, vb = zero;
    if (two) {
      gb = g4[i2];
      pb = p4[i2];
      mb = m4[i2];
      if (adam) vb = v4[i2];
    }
    opt_update(hp, c, coef, ga.x, pa.x, ma.x, va.x);
    opt_update(hp, c, coef, ga.y, pa.y, ma.y, va.y);
    opt_update(hp, c, coef, ga.z, pa.z, ma.z, va.z);
    opt_update(hp, c, coef, ga.w, pa.w, ma.w, va.w);
    g4[i] = zero;
    p4[i] = pa;
    m4[i] = ma;
    if (adam) v4[i] = va;
    if (two) {
      opt_update(hp, c, coef, gb.x, pb.x, mb.x, vb.x);
      opt_update(hp, c, coef, gb.y, pb.y, mb.y, vb.y);
      opt_update(hp, c, coef, gb.z, pb.z, mb.z, vb.z);
      opt_update(hp, c, coef, gb.w, pb.w, mb.w, vb.w);
      g4[i2] = zero;
      p4[i2] = pb;
      m4[i2] = mb;
      if (adam) v4[i2] = vb;
    }
  }
  const int64_t nend = (sp.a0 - sp.begin) + (sp.end - sp.a1);
  for (int64_t k = gtid; k < nend; k += stride) {
    const int64_t i = span_end_index(sp, k);
    float pp = p[i], m = s1[i], vv = adam ? s2[i] : 0.f;
    const float graw = g[i];
    g[i] = 0.f;
    opt_update(hp, c, coef, graw, pp, m, vv);
    p[i] = pp;
    s1[i] = m;
    if (adam) s2[i] = vv;
  }
}

// a frozen run: its gradient is zeroed (the fused backward kernels may have written it); p, m and v
// are neither loaded nor stored
__device__ __forceinline__ void span_zero(float* __restrict__ g, const OptSpan& sp) {
  const int64_t stride = (int64_t)gridDim.x * OPT_THREADS;
  const int64_t gtid = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x;
  const int64_t nv = (sp.a1 - sp.a0) / OPT_VEC;
  float4* g4 = reinterpret_cast<float4*>(g + sp.a0);
  for (int64_t i = gtid; i < nv; i += stride) g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t nend = (sp.a0 - sp.begin) + (sp.end - sp.a1);
  for (int64_t k = gtid; k < nend; k += stride) g[span_end_index(sp, k)] = 0.f;
}

// run k's span clipped to [0, P) (the host validates the table; this keeps a bad one in bounds)
__device__ __forceinline__ OptSpan table_span(const rai_optim_run& r, int64_t P, int vec) {
  const int64_t b = r.begin < 0 ? 0 : r.begin;
  const int64_t e = r.end > P ? P : r.end;
  return run_span(b, e < b ? b : e, vec);
}

// ---- the flat form ---------------------------------------------------------------------------
__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_kernel(const float* __restrict__ g,
                                                                int64_t P, int aligned,
                                                                double* partial,
                                                                rai_train_state* state) {
  const OptSpan sp = {0, 0, aligned ? (P / OPT_VEC) * OPT_VEC : 0, P};
  publish_partial(span_sumsq(g, sp, 0.0), partial, state);
}

__global__ __launch_bounds__(OPT_THREADS) void clip_optim_kernel(
    float* __restrict__ p, float* __restrict__ g, float* __restrict__ s1, float* __restrict__ s2,
    int64_t P, const rai_optim_hparams* __restrict__ hpp, rai_train_state* state,
    const double* __restrict__ partial, int nparts, float* norms, int max_norms, int vec) {
  const rai_optim_hparams hp = *hpp;
  const float coef = clip_coef(hp, state, partial, nparts, norms, max_norms);
  const OptConsts c = opt_consts(hp, state->opt_step);
  const OptSpan sp = {0, 0, vec ? (P / OPT_VEC) * OPT_VEC : 0, P};
  span_update(p, g, s1, s2, sp, hp, c, coef);
}

// ---- the run-wise form: every block walks the run table (block-uniform reads) --------------------
__global__ __launch_bounds__(OPT_THREADS) void grad_sumsq_runs_kernel(
    const float* __restrict__ g, int64_t P, int aligned, const rai_optim_run* __restrict__ runs,
    int n_runs, double* partial, rai_train_state* state) {
  double s = 0.0;
  for (int k = 0; k < n_runs; ++k) {
    const rai_optim_run r = runs[k];
    if (r.active) s = span_sumsq(g, table_span(r, P, aligned), s);
  }
  publish_partial(s, partial, state);
}

__global__ __launch_bounds__(OPT_THREADS) void clip_optim_runs_kernel(
    float* __restrict__ p, float* __restrict__ g, float* __restrict__ s1, float* __restrict__ s2,
    int64_t P, const rai_optim_hparams* __restrict__ hpp, rai_train_state* state,
    const rai_optim_run* __restrict__ runs, int n_runs, const double* __restrict__ partial,
    int nparts, float* norms, int max_norms, int vec) {
  const rai_optim_hparams hp = *hpp;
  const float coef = clip_coef(hp, state, partial, nparts, norms, max_norms);
  const int64_t step = state->opt_step;
  for (int k = 0; k < n_runs; ++k) {
    const rai_optim_run r = runs[k];
    const OptSpan sp = table_span(r, P, vec);
    if (r.active)
      span_update(p, g, s1, s2, sp, hp, opt_consts(hp, step - r.lag), coef);
    else
      span_zero(g, sp);
  }
}

inline int opt_blocks(int64_t P) {
  int64_t b = (P + OPT_THREADS * 8 - 1) / (OPT_THREADS * 8);
  if (b < 1) b = 1;
  if (b > OPT_MAX_BLOCKS) b = OPT_MAX_BLOCKS;
  return (int)b;
}

}  // namespace

// The per-block fp64 partials.  Round 2's opt-in one-launch form (an in-kernel arrival barrier
// over every workgroup) measured no faster (profiles/r2zs_optim_ab.txt) and could leave a partial
// step when a workgroup was held off the GPU past its bounded wait; it was removed in round 3.
extern "C" int64_t rai_optim_workspace_bytes(int64_t /*P*/) {
  return (int64_t)OPT_MAX_BLOCKS * sizeof(double);
}

extern "C" int rai_clip_optim_step(float* params, float* grads, float* state1, float* state2,
                                   int64_t P, const rai_optim_hparams* hp, rai_train_state* state,
                                   float* norms, int32_t max_norms, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  if (P < 1) return RAI_E_SHAPE;
  if (!params || !grads || !state1 || !hp || !state || !workspace) return RAI_E_NULLPTR;
  if (workspace_bytes < rai_optim_workspace_bytes(P)) return RAI_E_WORKSPACE;
  if (!state2) state2 = state1;  // RMSprop uses one state buffer
  const int blocks = opt_blocks(P);
  double* partial = reinterpret_cast<double*>(workspace);
  const int aligned = ((uintptr_t)grads % 16) == 0;
  const int vec = aligned && ((uintptr_t)params % 16) == 0 && ((uintptr_t)state1 % 16) == 0 &&
                  ((uintptr_t)state2 % 16) == 0;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(OPT_THREADS), 0, rai_stream(stream),
                     grads, P, aligned, partial, state);
  RAI_LAUNCH_CHECK();
  hipLaunchKernelGGL(clip_optim_kernel, dim3(blocks), dim3(OPT_THREADS), 0, rai_stream(stream),
                     params, grads, state1, state2, P, hp, state, partial, blocks, norms,
                     max_norms, vec);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_clip_optim_step_runs(float* params, float* grads, float* state1, float* state2,
                                        int64_t P, const rai_optim_hparams* hp,
                                        rai_train_state* state, const rai_optim_run* runs,
                                        int32_t n_runs, float* norms, int32_t max_norms,
                                        void* workspace, int64_t workspace_bytes, void* stream) {
  if (P < 1 || n_runs < 1 || n_runs > RAI_OPTIM_MAX_RUNS) return RAI_E_SHAPE;
  if (!params || !grads || !state1 || !hp || !state || !workspace || !runs) return RAI_E_NULLPTR;
  if (workspace_bytes < rai_optim_workspace_bytes(P)) return RAI_E_WORKSPACE;
  if (!state2) state2 = state1;
  const int blocks = opt_blocks(P);
  double* partial = reinterpret_cast<double*>(workspace);
  const int aligned = ((uintptr_t)grads % 16) == 0;
  const int vec = aligned && ((uintptr_t)params % 16) == 0 && ((uintptr_t)state1 % 16) == 0 &&
                  ((uintptr_t)state2 % 16) == 0;
  hipLaunchKernelGGL(grad_sumsq_runs_kernel, dim3(blocks), dim3(OPT_THREADS), 0, rai_stream(stream),
                     grads, P, aligned, runs, n_runs, partial, state);
  RAI_LAUNCH_CHECK();
  hipLaunchKernelGGL(clip_optim_runs_kernel, dim3(blocks), dim3(OPT_THREADS), 0, rai_stream(stream),
                     params, grads, state1, state2, P, hp, state, runs, n_runs, partial, blocks,
                     norms, max_norms, vec);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

int rai_internal::optim_apply_partials(float* params, float* grads, float* state1, float* state2, int64_t P,
                                       const rai_optim_hparams* hp, rai_train_state* state, const double* partial,
                                       int nparts, float* norms, int32_t max_norms, hipStream_t stream) {
  if (P < 1 || nparts < 1) return RAI_E_SHAPE;
  if (!params || !grads || !state1 || !hp || !state || !partial) return RAI_E_NULLPTR;
  if (!state2) state2 = state1;
  const int vec = ((uintptr_t)grads % 16) == 0 && ((uintptr_t)params % 16) == 0 && ((uintptr_t)state1 % 16) == 0 &&
                  ((uintptr_t)state2 % 16) == 0;
  hipLaunchKernelGGL(clip_optim_kernel, dim3(opt_blocks(P)), dim3(OPT_THREADS), 0, stream, params, grads, state1,
                     state2, P, hp, state, partial, nparts, norms, max_norms, vec);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}
