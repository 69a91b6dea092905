// Fused PPO epoch for small MLP actor-critics on gfx950 (CartPole-class policies).
//
// One launch runs EVERY minibatch of one epoch of rl_algo_impls/ppo/ppo.py:290-411
// for an ActorCritic whose encoder is Flatten and whose actor/critic heads are
// [in -> 64 -> 64 -> out] MLPs (rl_algo_impls/shared/policy/actor_critic_network/
// connected_trio.py + shared/actor/categorical.py + shared/policy/critic.py):
//   forward, categorical logp/entropy, clipped-surrogate + value loss gradients,
//   backward, clip_grad_norm_ and Adam(eps) — without leaving the chip.
//
// Why one launch: at the CartPole config an update is 40,960 *dependent* Adam steps
// of ~13 MFLOP each; per-step launches cost more than the arithmetic.  Advantage
// normalisation moments (ppo.py:313-316) are computed for all the epoch's minibatches
// by a small pre-kernel, off the dependent chain.
//
// This file holds the kernels' argument block (MlpArgs), the choice of kernel, the launch
// and the exported entry points.  The kernels are in the headers included below:
//   mlp_mc8.h        8 or 16 CUs per network: the default for the CartPole class (in_dim <= 4,
//                    n_actions <= 2), and the only one with the in-kernel cross-GPU exchange
//   mlp_mc.h         4 CUs per network: the data-parallel grads / apply step (RAI_MLP_LAYOUT=mc4:
//                    epoch mode too)
//   mlp_net.h        one CU per network: shapes up to (8, 8) (RAI_MLP_LAYOUT=chunk: CartPole too)
//   mlp_mc_common.h  what they share: the small device helpers, clip coefficient, stat rows, weight
//                    layout, exchange region, weight / moment load and write-back
//   ppo_row_loss.h   the per-row loss and its gradient (the surrogate and value terms: ppo_terms.h)
#include "common.h"
#include "internal.h"
#include "ppo_terms.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#pragma clang fp contract(off)

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

constexpr int HID = 64;
constexpr int LD = 66;
constexpr int CH = 128;
constexpr int MAXIN = 8;
constexpr int MAXOUT = 8;
constexpr int MAXB = 256;
constexpr int NT = 1024;
constexpr int NW = NT / 64;

struct MlpArgs {
  float* params;
  float* exp_avg;
  float* exp_avg_sq;
  const float* obs;
  const int64_t* actions;
  const float* old_logp;
  const float* old_values;
  const float* adv;
  const float* ret;
  int64_t n_rows;
  int32_t batch;
  int32_t in_dim;
  int32_t n_act;
  int32_t act_fn;
  const rai_ppo_hparams* hp;
  const rai_optim_hparams* ohp;
  rai_train_state* state;
  float* stats;
  int32_t max_stats;
  float* norms;
  int32_t max_norms;
  unsigned long long* xchg;  // [0..3]: [2 nets][2 parities]; [4]: critic-done flag; zeroed per launch
  int32_t* err;
  // per-minibatch (mean, den) of the advantage normalisation: moments[2*mb], moments[2*mb+1]
  const float* moments;
  // multi-CU layout: the exchange slots (workspace)
  float* scratch;
  // multi-CU layout: per-CU loss-statistic partials [2 nets][minibatches][MC_G][4] (workspace)
  double* statp;
  // data-parallel "grads" mode (grad_out != nullptr): process minibatches
  // [mb_begin, mb_begin + mb_count), scale the loss means by 1/(rows*world), write the
  // raw gradients to grad_out and stop (the caller all-reduces them and runs
  // rai_clip_optim_step).
  float* grad_out;
  int32_t mb_begin;
  int32_t mb_count;
  int32_t world;
  // multi-CU data-parallel step (grads mode only): before the minibatch, apply clip_grad_norm_ +
  // Adam with the all-reduced flat gradient of the previous step (grad_in, P_total elements: both
  // networks); sync_base = number of earlier launches since the sync words were last zeroed
  const float* grad_in;
  int32_t P_total;
  int32_t sync_base;
  // in-kernel cross-GPU exchange (multi-CU layout, epoch mode): xpeers[r] = rank r's exchange
  // region (IPC-mapped device memory, uncached), xbase = optimizer steps already exchanged
  // through these regions (flags are monotonic step ids, never re-zeroed)
  void* const* xpeers;
  int32_t xrank;
  int32_t xworld;
  int64_t xbase;
};

#include "ppo_row_loss.h"
#include "mlp_mc_common.h"
#include "mlp_net.h"
#include "mlp_mc.h"
#include "mlp_mc8.h"

// Advantage-normalisation moments of every minibatch (one workgroup per minibatch), in the
// operation order of the loss kernel: fp64 sums, mean rounded to f32, unbiased std
// (ppo.py:313-316: (A - A.mean()) / (A.std() + 1e-8); standardize: A / (A.std() + 1e-8)).
__global__ __launch_bounds__(256) void adv_moments_kernel(const float* __restrict__ adv, int64_t n_rows, int B,
                                                          const rai_ppo_hparams* hp, float* moments) {
  __shared__ double scratch[4];
  const int mb = blockIdx.x;
  const int64_t row0 = (int64_t)mb * B;
  const int rows = (int)min((int64_t)B, n_rows - row0);
  const int tid = threadIdx.x;
  const float x = tid < rows ? adv[row0 + tid] : 0.f;
  double v1[1] = {tid < rows ? (double)x : 0.0};
  block_sum<1>(v1, scratch);
  const float mean = (float)(v1[0] / (double)rows);
  const double d = tid < rows ? (double)x - (double)mean : 0.0;
  double v2[1] = {d * d};
  block_sum<1>(v2, scratch);
  if (tid == 0) {
    const float den = (float)sqrt(v2[0] / (double)(rows - 1)) + 1e-8f;
    float m0 = 0.f, m1 = 1.f;
    if (hp->normalize_advantage) { m0 = mean; m1 = den; }
    else if (hp->standardize_advantage) { m1 = den; }
    moments[2 * mb] = m0;
    moments[2 * mb + 1] = m1;
  }
}

constexpr int64_t XCHG_BYTES = 256;  // exchange words (first 64 B zeroed per launch), padded
constexpr int64_t SCRATCH_MC = 2LL * 2 * MC_G * MC_SLOT * sizeof(float);
constexpr int64_t SCRATCH_BYTES = SCRATCH_MC > M8_SCRATCH ? SCRATCH_MC : M8_SCRATCH;

// The CartPole class: the shapes the multi-CU kernels take (observations padded to 4, two logits)
bool mlp_cartpole_class(int32_t in_dim, int32_t n_act) { return in_dim <= 4 && n_act <= 2; }

// Kernel layout for the CartPole class (diagnostics / A-B only: RAI_MLP_LAYOUT=chunk|mc4)
enum MlpLayout {
  LAYOUT_DEFAULT,  // multi-CU: 8 or 16 CUs per network (epoch mode), 4 (data-parallel grads mode)
  LAYOUT_CHUNK,    // one CU per network
  LAYOUT_MC4,      // 4 CUs per network in epoch mode too
};
MlpLayout mlp_layout() {
  const char* e = getenv("RAI_MLP_LAYOUT");
  if (e && !strcmp(e, "chunk")) return LAYOUT_CHUNK;
  if (e && !strcmp(e, "mc4")) return LAYOUT_MC4;
  return LAYOUT_DEFAULT;
}

// CUs per network of the default epoch kernel (A-B: RAI_MLP_CUS=8|16)
int mlp_cus_per_net() {
  const char* e = getenv("RAI_MLP_CUS");
  return (e && !strcmp(e, "8")) ? 8 : 16;
}

// Per-rank geometry for minibatches of <= 128 rows (A-B: RAI_MLP_PER_RANK_GEO=0 keeps 16 CUs)
bool mlp_per_rank_geometry() {
  const char* e = getenv("RAI_MLP_PER_RANK_GEO");
  return !(e && !strcmp(e, "0"));
}

int64_t num_minibatches(int64_t n_rows, int32_t batch_size) {
  return batch_size > 0 ? (n_rows + batch_size - 1) / batch_size : 0;
}
int64_t moments_bytes(int64_t n_rows, int32_t batch_size) {
  return ((8 * num_minibatches(n_rows, batch_size) + 255) / 256) * 256;
}
int64_t statp_bytes(int64_t n_rows, int32_t batch_size) {
  return 2 * num_minibatches(n_rows, batch_size) * (MC_G > M8_GMAX ? MC_G : M8_GMAX) * 4 * (int64_t)sizeof(double);
}

// The fields every entry point fills the same way: an epoch over all minibatches on one GPU with
// advantage moments computed here (each entry point then sets what differs)
MlpArgs mlp_args(float* params, float* exp_avg, float* exp_avg_sq, const float* obs, const int64_t* actions,
                 const float* old_logp, const float* old_values, const float* advantages, const float* returns,
                 int32_t in_dim, int32_t n_actions, int32_t activation, const rai_ppo_hparams* hp,
                 const rai_optim_hparams* ohp, rai_train_state* state, float* stats, int32_t max_stats, float* norms,
                 int32_t max_norms) {
  MlpArgs a = {};
  a.params = params; a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq;
  a.obs = obs; a.actions = actions; a.old_logp = old_logp; a.old_values = old_values;
  a.adv = advantages; a.ret = returns;
  a.in_dim = in_dim; a.n_act = n_actions; a.act_fn = activation;
  a.hp = hp; a.ohp = ohp; a.state = state;
  a.stats = stats; a.max_stats = max_stats; a.norms = norms; a.max_norms = max_norms;
  a.mb_begin = 0; a.mb_count = 1 << 30; a.world = 1;
  return a;
}

// Which epoch kernel a launch runs, and its geometry
struct MlpKernel {
  void (*relu)(const MlpArgs), (*tanh)(const MlpArgs);  // the act_fn 1 and act_fn 0 instantiations
  int grid, threads;
};
MlpKernel mlp_kernel(const MlpArgs& a, int32_t batch_size) {
  if (!mlp_cartpole_class(a.in_dim, a.n_act)) return {mlp_ppo_epoch_kernel<8, 8, 1>, mlp_ppo_epoch_kernel<8, 8, 0>, 2, NT};
  const MlpLayout layout = mlp_layout();
  if (layout == LAYOUT_CHUNK) return {mlp_ppo_epoch_kernel<4, 2, 1>, mlp_ppo_epoch_kernel<4, 2, 0>, 2, NT};
  // MC_G CUs per network, partial-gradient all-reduce per minibatch: the data-parallel grads step
  if (a.grad_out || layout == LAYOUT_MC4) return {mlp_ppo_mc_kernel<1>, mlp_ppo_mc_kernel<0>, MC_GRID, MC_NT};
  // G CUs per network: reduce-scatter + all-gather per minibatch
  if (mlp_cus_per_net() == 8) return {mlp_ppo_mc8_kernel<1, 8>, mlp_ppo_mc8_kernel<0, 8>, M8Geo<8>::GRID, MC_NT};
  // <= 128 rows (256 / world per rank at world 2): 8 CUs of 16 rows, not 16 CUs of which half hold no rows
  if (batch_size <= 128 && mlp_per_rank_geometry())
    return {mlp_ppo_mc8_kernel<1, 8, 16>, mlp_ppo_mc8_kernel<0, 8, 16>, M8Geo<8, 16>::GRID, MC_NT};
  return {mlp_ppo_mc8_kernel<1, 16>, mlp_ppo_mc8_kernel<0, 16>, M8Geo<16>::GRID, MC_NT};
}

int mlp_launch(MlpArgs& a, int32_t hidden, int32_t batch_size, int64_t n_rows, void* workspace,
               int64_t workspace_bytes, void* stream) {
  if (hidden != HID || a.in_dim < 1 || a.in_dim > MAXIN || a.n_act < 1 || a.n_act > MAXOUT ||
      batch_size < 2 || batch_size > MAXB || n_rows < 1 || (a.act_fn != 0 && a.act_fn != 1) ||
      a.world < 1)
    return RAI_E_SHAPE;
  if (!a.params || !a.obs || !a.actions || !a.old_logp || !a.old_values || !a.adv || !a.ret ||
      !a.hp || !a.ohp || !a.state || !workspace)
    return RAI_E_NULLPTR;
  if (!a.grad_out && (!a.exp_avg || !a.exp_avg_sq)) return RAI_E_NULLPTR;
  if (workspace_bytes < rai_mlp_ppo_workspace_bytes(n_rows, batch_size)) return RAI_E_WORKSPACE;
  if (n_rows % batch_size == 1 && !a.moments) return RAI_E_SHAPE;  // 1-row minibatch: no std
  if (a.grad_out && a.mb_count > 0 && (int64_t)a.mb_begin * batch_size >= n_rows) return RAI_E_SHAPE;
  a.n_rows = n_rows;
  a.batch = batch_size;
  a.xchg = reinterpret_cast<unsigned long long*>(workspace);
  a.err = &a.state->err;
  hipStream_t s = rai_stream(stream);
  if (a.sync_base == 0) {  // later launches of a data-parallel epoch keep counting on the same words
    hipError_t e = hipMemsetAsync(workspace, 0, XCHG_BYTES, s);
    if (e != hipSuccess) return (int)e;
  }
  a.scratch = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + XCHG_BYTES);
  if (!a.moments) {
    float* mom = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + XCHG_BYTES + SCRATCH_BYTES);
    const int64_t nmb = num_minibatches(n_rows, batch_size);
    hipLaunchKernelGGL(adv_moments_kernel, dim3((unsigned)nmb), dim3(256), 0, s, a.adv, n_rows, batch_size, a.hp,
                       mom);
    RAI_LAUNCH_CHECK();
    a.moments = mom;
  }
  a.statp = reinterpret_cast<double*>(static_cast<unsigned char*>(workspace) + XCHG_BYTES + SCRATCH_BYTES +
                                      moments_bytes(n_rows, batch_size));
  const MlpKernel k = mlp_kernel(a, batch_size);
  hipLaunchKernelGGL(a.act_fn == 1 ? k.relu : k.tanh, dim3(k.grid), dim3(k.threads), 0, s, a);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}
}  // namespace

#ifdef RAI_STAMPS
extern "C" int rai_mlp_debug_stamps(unsigned long long* host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), sizeof(g_stamps));
}
#endif

extern "C" int64_t rai_mlp_ppo_workspace_bytes(int64_t n_rows, int32_t batch_size) {
  if (batch_size > MAXB) return rai_internal::mlp_large_workspace_bytes(n_rows, batch_size);
  return XCHG_BYTES + SCRATCH_BYTES + moments_bytes(n_rows, batch_size) + statp_bytes(n_rows, batch_size);
}

extern "C" int rai_mlp_ppo_epoch(float* params, float* exp_avg, float* exp_avg_sq, const float* obs,
                                 const int64_t* actions, const float* old_logp, const float* old_values,
                                 const float* advantages, const float* returns, int64_t n_rows,
                                 int32_t batch_size, int32_t in_dim, int32_t hidden, int32_t n_actions,
                                 int32_t activation, const rai_ppo_hparams* hp, const rai_optim_hparams* ohp,
                                 rai_train_state* state, float* stats, int32_t max_stats, float* norms,
                                 int32_t max_norms, void* workspace, int64_t workspace_bytes,
                                 void* stream) {
  if (batch_size > MAXB) {  // SURVEY 8(d) batch policy (b): the all-CU large-minibatch step (mlp_large.hip)
    if (!rai_internal::mlp_large_supported(in_dim, n_actions, hidden)) return RAI_E_UNSUPPORTED;
    return rai_internal::mlp_large(params, exp_avg, exp_avg_sq, obs, actions, old_logp, old_values, advantages,
                                   returns, n_rows, batch_size, in_dim, n_actions, activation, 0, 1 << 30, nullptr,
                                   1, hp, ohp, state, stats, max_stats, norms, max_norms, nullptr, workspace,
                                   workspace_bytes, rai_stream(stream));
  }
  MlpArgs a = mlp_args(params, exp_avg, exp_avg_sq, obs, actions, old_logp, old_values, advantages, returns, in_dim,
                       n_actions, activation, hp, ohp, state, stats, max_stats, norms, max_norms);
  return mlp_launch(a, hidden, batch_size, n_rows, workspace, workspace_bytes, stream);
}

extern "C" int rai_mlp_ppo_epoch_xdp(float* params, float* exp_avg, float* exp_avg_sq, const float* obs,
                                     const int64_t* actions, const float* old_logp, const float* old_values,
                                     const float* advantages, const float* returns, int64_t n_rows,
                                     int32_t batch_size, const float* moments, int32_t world, int32_t rank,
                                     void* const* peers, int64_t step_base, int32_t in_dim, int32_t hidden,
                                     int32_t n_actions, int32_t activation, const rai_ppo_hparams* hp,
                                     const rai_optim_hparams* ohp, rai_train_state* state, float* stats,
                                     int32_t max_stats, float* norms, int32_t max_norms, void* workspace,
                                     int64_t workspace_bytes, void* stream) {
  if (!moments || !peers) return RAI_E_NULLPTR;
  if (world < 2 || world > XDP_MAXW || rank < 0 || rank >= world || step_base < 0) return RAI_E_SHAPE;
  if (batch_size > MAXB) {  // large minibatches (mlp_large.hip): the exchange inside each step's reduce launch
    if (!rai_internal::mlp_large_supported(in_dim, n_actions, hidden)) return RAI_E_UNSUPPORTED;
    const rai_internal::LargeXdp x = {peers, rank, world, step_base};
    return rai_internal::mlp_large(params, exp_avg, exp_avg_sq, obs, actions, old_logp, old_values, advantages,
                                   returns, n_rows, batch_size, in_dim, n_actions, activation, 0, 1 << 30, moments,
                                   world, hp, ohp, state, stats, max_stats, norms, max_norms, nullptr, workspace,
                                   workspace_bytes, rai_stream(stream), &x);
  }
  // the in-kernel exchange is the default epoch kernel's (mlp_mc8.h): the diagnostic layouts have none
  if (!mlp_cartpole_class(in_dim, n_actions) || mlp_layout() != LAYOUT_DEFAULT) return RAI_E_UNSUPPORTED;
  MlpArgs a = mlp_args(params, exp_avg, exp_avg_sq, obs, actions, old_logp, old_values, advantages, returns, in_dim,
                       n_actions, activation, hp, ohp, state, stats, max_stats, norms, max_norms);
  a.moments = moments; a.world = world;
  a.xpeers = peers; a.xrank = rank; a.xworld = world; a.xbase = step_base;
  return mlp_launch(a, hidden, batch_size, n_rows, workspace, workspace_bytes, stream);
}

// Setup-time canary for the cross-GPU regions: the same memory, scopes and flag protocol as
// the epoch kernel on a known payload.  bad[0] counts wrong values, bad[1] timeouts.
__global__ __launch_bounds__(64) void xdp_selftest_kernel(void* const* peers, int W, int rank,
                                                          unsigned long long tag, int* bad) {
  const int lane = threadIdx.x;
  for (int p = 0; p < W; ++p) {
    float* dst = reinterpret_cast<float*>(static_cast<char*>(peers[p]) + XDP_FLAGS_BYTES) + rank * 64 + lane;
    __hip_atomic_store(dst, (float)(rank * 1000 + lane) + (float)tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (lane < W) {
    unsigned long long* fl = reinterpret_cast<unsigned long long*>(static_cast<char*>(peers[lane]) + XDP_TEST_OFF) + rank;
    __hip_atomic_store(fl, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const unsigned long long* own = reinterpret_cast<const unsigned long long*>(static_cast<char*>(peers[rank]) + XDP_TEST_OFF);
  unsigned long long spins = 0;
  for (;;) {
    bool ok = lane >= W || __hip_atomic_load(own + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >= tag;
    if (__all(ok)) break;
    if (++spins > (1ull << 22)) {
      if (lane == 0) atomicAdd(&bad[1], 1);
      return;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  const float* src = reinterpret_cast<const float*>(static_cast<const char*>(peers[rank]) + XDP_FLAGS_BYTES);
  for (int r = 0; r < W; ++r) {
    const float v = __hip_atomic_load(src + r * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (v != (float)(r * 1000 + lane) + (float)tag) atomicAdd(&bad[0], 1);
  }
}

extern "C" int rai_xdp_selftest(void* const* peers, int32_t world, int32_t rank, int64_t tag, int32_t* bad,
                                void* stream) {
  if (!peers || !bad) return RAI_E_NULLPTR;
  if (world < 1 || world > XDP_MAXW || rank < 0 || rank >= world || tag < 1) return RAI_E_SHAPE;
  hipLaunchKernelGGL(xdp_selftest_kernel, dim3(1), dim3(64), 0, rai_stream(stream), peers, (int)world, (int)rank,
                     (unsigned long long)tag, bad);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int64_t rai_xdp_region_bytes(int32_t world) {
  if (world < 1 || world > XDP_MAXW) return 0;
  static_assert(XDP_FLAGS_BYTES == RAI_XDP_SLOTS_OFF, "one region layout");
  // one region serves the CartPole-class epoch kernels (<= 256 rows and the large-minibatch steps) and the
  // wide whole-epoch kernel
  return std::max<int64_t>(std::max<int64_t>(xdp_region_bytes(world), rai_xdp_wide_bytes(world)),
                           rai_internal::mlp_large_xdp_bytes(world));
}

// Multi-CU data-parallel step (used by rai_mlp_ppo_epoch_dp): apply the previous all-reduced
// gradient (grad_in; nullptr on the first step) then compute minibatch mb's partial gradient into
// grad_out (mb_count 0: apply only).  Returns RAI_E_UNSUPPORTED for shapes outside the multi-CU
// layout; the caller then uses the three-call sequence.
int rai_mlp_ppo_dp_step(float* params, float* exp_avg, float* exp_avg_sq, const float* grad_in, int32_t P_total,
                        const float* obs, const int64_t* actions, const float* old_logp, const float* old_values,
                        const float* advantages, const float* returns, int64_t n_rows, int32_t batch_size,
                        int32_t mb, int32_t mb_count, const float* moments, int32_t world, int32_t in_dim,
                        int32_t hidden, int32_t n_actions, int32_t activation, const rai_ppo_hparams* hp,
                        const rai_optim_hparams* ohp, rai_train_state* state, float* grad_out, float* stats,
                        int32_t max_stats, float* norms, int32_t max_norms, int32_t sync_base, void* workspace,
                        int64_t workspace_bytes, void* stream) {
  if (!mlp_cartpole_class(in_dim, n_actions) || mlp_layout() == LAYOUT_CHUNK || batch_size > MAXB)
    return RAI_E_UNSUPPORTED;
  if (!grad_out || !moments || !exp_avg || !exp_avg_sq) return RAI_E_NULLPTR;
  if (mb < 0 || mb_count < 0 || sync_base < 0) return RAI_E_SHAPE;
  MlpArgs a = mlp_args(params, exp_avg, exp_avg_sq, obs, actions, old_logp, old_values, advantages, returns, in_dim,
                       n_actions, activation, hp, ohp, state, stats, max_stats, norms, max_norms);
  a.grad_out = grad_out; a.moments = moments;
  a.mb_begin = mb; a.mb_count = mb_count; a.world = world;
  a.grad_in = grad_in; a.P_total = P_total; a.sync_base = sync_base;
  return mlp_launch(a, hidden, batch_size, n_rows, workspace, workspace_bytes, stream);
}

extern "C" int rai_mlp_ppo_grads(const float* params, const float* obs, const int64_t* actions,
                                 const float* old_logp, const float* old_values,
                                 const float* advantages, const float* returns, int64_t n_rows,
                                 int32_t batch_size, int32_t mb_begin, int32_t mb_count,
                                 const float* moments, int32_t world, int32_t in_dim, int32_t hidden,
                                 int32_t n_actions, int32_t activation, const rai_ppo_hparams* hp,
                                 const rai_optim_hparams* ohp, rai_train_state* state, float* grad_out,
                                 float* stats, int32_t max_stats, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
  if (!grad_out) return RAI_E_NULLPTR;
  if (mb_begin < 0 || mb_count < 1) return RAI_E_SHAPE;
  if (batch_size > MAXB) {  // large minibatches: one minibatch per call (mlp_large.hip)
    if (!rai_internal::mlp_large_supported(in_dim, n_actions, hidden)) return RAI_E_UNSUPPORTED;
    return rai_internal::mlp_large(const_cast<float*>(params), nullptr, nullptr, obs, actions, old_logp, old_values,
                                   advantages, returns, n_rows, batch_size, in_dim, n_actions, activation, mb_begin,
                                   mb_count, moments, world, hp, ohp, state, stats, max_stats, nullptr, 0, grad_out,
                                   workspace, workspace_bytes, rai_stream(stream));
  }
  // no optimizer state and no norms: the caller all-reduces grad_out and runs rai_clip_optim_step
  MlpArgs a = mlp_args(const_cast<float*>(params), nullptr, nullptr, obs, actions, old_logp, old_values, advantages,
                       returns, in_dim, n_actions, activation, hp, ohp, state, stats, max_stats, nullptr, 0);
  a.grad_out = grad_out; a.moments = moments;
  a.mb_begin = mb_begin; a.mb_count = mb_count; a.world = world;
  return mlp_launch(a, hidden, batch_size, n_rows, workspace, workspace_bytes, stream);
}
