// The per-row PPO loss and its gradient, shared by every 64-wide fused epoch kernel (mlp_net, mlp_mc,
// mlp_mc8).  Included once, inside mlp_ppo.hip's anonymous namespace, before any kernel body; compiled
// under that file's fp contract(off).

constexpr float F32_MIN = -3.4028234663852886e38f;

__device__ __forceinline__ float vf_loss(int fn, float x) {
  if (fn == 0) return x * x;
  const float z = fabsf(x);
  return z < 1.f ? 0.5f * z * z : (z - 0.5f);
}
__device__ __forceinline__ float vf_grad(int fn, float x) {
  if (fn == 0) return 2.f * x;
  return x <= -1.f ? -1.f : (x >= 1.f ? 1.f : x);
}

// Per-row PPO loss gradient (reference: rl_algo_impls/ppo/ppo.py:326-377; autograd's tie rules of
// min / max and the closed-interval clamp, as loss.hip) for one row's logits (actor) or value
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
    float m = F32_MIN;
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
        H -= fmaxf(n, F32_MIN) * expf(n);
      }
    const int act = min(max(c_act, 0), NA - 1);
    float zact = z[0];
#pragma unroll
    for (int o = 1; o < OUTP; ++o)
      if (o == act) zact = z[o];
    const float logp = zact - lse;
    const float logratio = logp - c_a;
    const float ratio = expf(logratio);
    const float lo = 1.f - h.clip_range, hi = 1.f + h.clip_range;
    const float cr = fminf(fmaxf(ratio, lo), hi);
    const float s1 = ratio * A, s2 = cr * A;
    const float gpi = -h.pi_coef * h.invB;
    float g1, g2;
    if (s1 < s2) { g1 = gpi; g2 = 0.f; }
    else if (s1 > s2) { g1 = 0.f; g2 = gpi; }
    else { g1 = gpi * 0.5f; g2 = gpi * 0.5f; }
    const float in_clip = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
    const float dlogp = (g1 * A + (g2 * A) * in_clip) * ratio;
    const float dent = -h.ent_coef * h.invB;
#pragma unroll
    for (int o = 0; o < OUTP; ++o)
      if (o < NA) {
        const float n = z[o] - lse;
        const float p = expf(n);
        dq[o] = dlogp * ((o == act ? 1.f : 0.f) - p) + dent * (-p * (n + H));
      }
    st[0] = fminf(s1, s2);
    st[1] = (ratio - 1.f) - logratio;
    st[2] = (fabsf(ratio - 1.f) > h.clip_range) ? 1.f : 0.f;
    st[3] = H;
  } else {
    const float v = z[0], Rt = c_b;
    const float gl = (h.vf_coef0 * h.halve) * h.invB;
    float l = vf_loss(h.vf_fn, v - Rt), dv;
    float vcf = 0.f;
    if (h.has_vclip) {
      const float vc_ = h.clip_range_vf;
      const float dvo = v - c_a;
      const float vcl = c_a + fminf(fmaxf(dvo, -vc_), vc_);
      const float l2 = vf_loss(h.vf_fn, vcl - Rt);
      float w1, w2;
      if (l > l2) { w1 = gl; w2 = 0.f; }
      else if (l < l2) { w1 = 0.f; w2 = gl; }
      else { w1 = gl * 0.5f; w2 = gl * 0.5f; }
      const float inv = (dvo >= -vc_ && dvo <= vc_) ? 1.f : 0.f;
      dv = w1 * vf_grad(h.vf_fn, v - Rt) + (w2 * vf_grad(h.vf_fn, vcl - Rt)) * inv;
      vcf = (fabsf(v - c_a) > vc_) ? 1.f : 0.f;
      l = fmaxf(l, l2);
    } else {
      dv = gl * vf_grad(h.vf_fn, v - Rt);
    }
    dq[0] = dv;
    st[0] = l;
    st[1] = vcf;
  }
}
