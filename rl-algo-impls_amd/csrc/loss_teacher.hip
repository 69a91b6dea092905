// The PPO loss with the teacher-KL term (rai_ppo_loss_teacher): loss_body.h's row loop with its
// TEACHER switch on.
//
// Restates, per minibatch, on top of what loss.hip restates:
//   rl_algo_impls/loss/teacher_kl_loss.py:35-50  the row term, (exp(d) - 1) - d or 0.5 d^2 with
//                                                d = teacher_logp - new_logp, weighted by the ratio
//   rl_algo_impls/ppo/ppo.py:363-371             coef * mean(row) added to the loss (before the
//                                                gradient-accumulation division; pi_coef does not
//                                                touch it), the un-scaled term kept as a stat
// and adds d(coef * mean(row)) / d(new_logp) to d_logp, the ratio's own dependence on new_logp
// included (the reference does not detach it).
//
// A file of its own, not a second kernel in loss.hip: the inliner's choices for the helpers a
// translation unit shares depend on how many kernels call them, so a kernel added to loss.hip changes
// the code of the ones already there.  Same launch geometry as rai_ppo_loss.
#include "common.h"
#include "ppo_terms.h"

namespace {

#include "loss_body.h"

template <int KM>
__global__ __launch_bounds__(LOSS_THREADS) void pg_loss_teacher_kernel(const TeacherLossArgs a) {
  pg_loss_body<KM, true>(a);
}

}  // namespace

extern "C" int rai_ppo_loss_teacher(const float* new_logp, const float* entropy, int64_t n_entropy,
                                    const float* new_values, const float* old_logp,
                                    const float* old_values, const float* advantages,
                                    const float* returns, int64_t B, int32_t K, const rai_ppo_hparams* hp,
                                    rai_train_state* state, float* d_logp, float* d_entropy,
                                    float* d_values, float* stats, int32_t max_stats,
                                    const float* teacher_logp, const rai_teacher_kl* tk,
                                    float* teacher_stats, int32_t loss_kind, void* /*workspace*/,
                                    int64_t /*workspace_bytes*/, void* stream) {
  if (B < 1 || K < 1 || n_entropy < 1) return RAI_E_SHAPE;
  if (K > RAI_MAX_K) return RAI_E_TOO_MANY_COLUMNS;
  if (!new_logp || !entropy || !new_values || !advantages || !returns || !hp || !state ||
      !d_logp || !d_entropy || !d_values || !teacher_logp || !tk)
    return RAI_E_NULLPTR;
  // the term is PPO's: it needs the rollout's log-probabilities for its ratio
  if (loss_kind != 0 || !old_logp) return RAI_E_MODE;
  TeacherLossArgs a;
  a.new_logp = new_logp;
  a.entropy = entropy;
  a.new_values = new_values;
  a.old_logp = old_logp;
  a.old_values = old_values ? old_values : new_values;
  a.adv = advantages;
  a.ret = returns;
  a.hp = hp;
  a.state = state;
  a.d_logp = d_logp;
  a.d_entropy = d_entropy;
  a.d_values = d_values;
  a.stats = stats;
  a.B = B;
  a.n_entropy = n_entropy;
  a.K = K;
  a.max_stats = max_stats;
  a.teacher_logp = teacher_logp;
  a.tk = tk;
  a.teacher_stats = teacher_stats;
  const unsigned nt = B <= 2048 ? 256u : (unsigned)LOSS_THREADS;
  if (K == 1) hipLaunchKernelGGL(pg_loss_teacher_kernel<1>, dim3(1), dim3(nt), 0, rai_stream(stream), a);
  else hipLaunchKernelGGL(pg_loss_teacher_kernel<RAI_MAX_K>, dim3(1), dim3(nt), 0, rai_stream(stream), a);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}
