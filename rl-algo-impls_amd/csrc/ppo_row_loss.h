// The per-row PPO loss and its gradient, shared by every 64-wide fused epoch kernel (mlp_net, mlp_mc,
// mlp_mc8).  Included once, inside mlp_ppo.hip's anonymous namespace, before any kernel body; compiled
// under that file's fp contract(off).  The clipped surrogate and the value term are ppo_terms.h's (which
// mlp_ppo.hip includes first); what is written here is the Categorical head around them: softmax,
// entropy and the gradient to the logits.

// Per-row PPO loss gradient (reference: rl_algo_impls/ppo/ppo.py:326-377; autograd's tie rules of
// min / max and the closed-interval clamp are in ppo_terms.h) for one row's logits (actor) or value
// (critic): dq = dLoss/dz, st = the row's statistics contributions (actor: surrogate, approx-KL
// term, clipped flag, entropy; critic: value loss, value-clipped flag).  A is the row's normalised
// advantage; c_a the old log-prob (actor) or old value (critic), c_b the return (critic).
// The hyperparameters are filled once per kernel from MlpArgs::hp; invB = 1 / (rows x world) per
// minibatch.
struct RowLossHp {
  float clip_range, ent_coef, pi_coef, invB, vf_coef0, halve, clip_range_vf;
  int has_vclip, vf_fn, NA;
};
// the launch-invariant fields; the kernel sets pi_coef (from the train state's latch) and invB
__device__ __forceinline__ RowLossHp row_loss_hp(const rai_ppo_hparams* hp, int NA) {
  RowLossHp h;
  h.clip_range = hp->clip_range;
  h.ent_coef = hp->ent_coef;
  h.vf_coef0 = hp->vf_coef[0];
  h.clip_range_vf = hp->clip_range_vf;
  h.has_vclip = hp->has_clip_range_vf;
  h.vf_fn = hp->vf_loss_fn;
  h.halve = hp->ppo2_vf_coef_halving ? 0.5f : 1.f;
  h.NA = NA;
  h.pi_coef = 1.f;
  h.invB = 0.f;
  return h;
}
template <int OUTP, bool ACTOR>
__device__ __forceinline__ void ppo_row_loss(const float (&z)[OUTP], const RowLossHp& h, int c_act, float c_a,
                                             float c_b, float A, float (&dq)[OUTP], float (&st)[4]) {
  if (ACTOR) {
    const int NA = h.NA;
    float m = RAI_F32_MIN;
#pragma unroll
    for (int o = 0; o < OUTP; ++o)
      if (o < NA) m = fmaxf(m, z[o]);
    float se = 0.f;
#pragma unroll
    for (int o = 0; o < OUTP; ++o)
      if (o < NA) se += expf(z[o] - m);
    const float lse = m + logf(se);
    float H = 0.f;
#pragma unroll
    for (int o = 0; o < OUTP; ++o)
      if (o < NA) {
        const float n = z[o] - lse;
        H -= fmaxf(n, RAI_F32_MIN) * expf(n);
      }
    const int act = min(max(c_act, 0), NA - 1);
    float zact = z[0];
#pragma unroll
    for (int o = 1; o < OUTP; ++o)
      if (o == act) zact = z[o];
    const PpoSurrogate s = ppo_surrogate(zact - lse, c_a, A, h.clip_range, -h.pi_coef * h.invB);
    const float dlogp = s.d_logp;
    const float dent = -h.ent_coef * h.invB;
#pragma unroll
    for (int o = 0; o < OUTP; ++o)
      if (o < NA) {
        const float n = z[o] - lse;
        const float p = expf(n);
        dq[o] = dlogp * ((o == act ? 1.f : 0.f) - p) + dent * (-p * (n + H));
      }
    st[0] = s.s_min;
    st[1] = s.kl_term;
    st[2] = s.clipped;
    st[3] = H;
  } else {
    const float gl = (h.vf_coef0 * h.halve) * h.invB;
    const PpoValue t = ppo_value_term(z[0], c_b, c_a, h.has_vclip != 0, h.clip_range_vf, h.vf_fn, gl);
    dq[0] = t.dv;
    st[0] = t.loss;
    st[1] = t.clipped;
  }
}
