// The PPO row terms (rl_algo_impls/ppo/ppo.py:326-361): the clipped surrogate and the optionally clipped
// value loss of one row, with their gradients under autograd's rules -- torch.min / torch.max split a tie
// 1/2 : 1/2 between their arguments, and clamp passes gradient on the closed interval.  The one place
// this arithmetic is written: ppo_row_loss.h (the 64-wide epoch kernels), loss_body.h (rai_ppo_loss,
// rai_ppo_loss_teacher, the wide head + loss kernel) and mlp_wide_epoch.hip call it.  Every function
// turns FP contraction off for itself, so the rounding sequence is the reference's whatever the including
// file is built with.  (mlp_large.hip keeps a contracted copy of its own; see its loss lambda.)
#ifndef RAI_PPO_TERMS_H
#define RAI_PPO_TERMS_H
#include "common.h"

// value-loss element: squared error (fn == 0) or Huber (smooth_l1, beta = 1) of x = v - R, and d/dx
__device__ __forceinline__ float vf_loss(int fn, float x) {
#pragma clang fp contract(off)
  if (fn == 0) return x * x;
  const float z = fabsf(x);
  return z < 1.f ? 0.5f * z * z : (z - 0.5f);
}
__device__ __forceinline__ float vf_grad(int fn, float x) {
#pragma clang fp contract(off)
  if (fn == 0) return 2.f * x;
  return x <= -1.f ? -1.f : (x >= 1.f ? 1.f : x);
}

// Policy term of one row.  g_pi = d loss / d min(s1, s2), formed by the caller; d_logp = d loss / d logp.
// s_min, kl_term ((ratio - 1) - logratio) and clipped are the row's statistics contributions.
struct PpoSurrogate {
  float ratio, logratio, s_min, kl_term, clipped, d_logp;
};
__device__ __forceinline__ PpoSurrogate ppo_surrogate(float logp, float old_logp, float A, float clip_range,
                                                      float g_pi) {
#pragma clang fp contract(off)
  PpoSurrogate s;
  s.logratio = logp - old_logp;
  s.ratio = expf(s.logratio);
  const float lo = 1.f - clip_range, hi = 1.f + clip_range;
  const float cr = fminf(fmaxf(s.ratio, lo), hi);
  const float s1 = s.ratio * A, s2 = cr * A;
  float g1, g2;
  if (s1 < s2) { g1 = g_pi; g2 = 0.f; }
  else if (s1 > s2) { g1 = 0.f; g2 = g_pi; }
  else { g1 = g_pi * 0.5f; g2 = g_pi * 0.5f; }
  const float in_clip = (s.ratio >= lo && s.ratio <= hi) ? 1.f : 0.f;
  s.d_logp = (g1 * A + (g2 * A) * in_clip) * s.ratio;
  s.s_min = fminf(s1, s2);
  s.kl_term = (s.ratio - 1.f) - s.logratio;
  s.clipped = fabsf(s.ratio - 1.f) > clip_range ? 1.f : 0.f;
  return s;
}

// Value term of one row and one value column.  gl = d loss / d (the row's value loss), formed by the
// caller; dv = d loss / d v.  loss is max(l, l2) under value clipping, l otherwise; clipped is then 0.
struct PpoValue {
  float loss, dv, clipped;
};
__device__ __forceinline__ PpoValue ppo_value_term(float v, float R, float v_old, bool has_vclip,
                                                   float clip_range_vf, int vf_fn, float gl) {
#pragma clang fp contract(off)
  PpoValue t;
  const float l = vf_loss(vf_fn, v - R);
  if (has_vclip) {
    const float dvo = v - v_old;
    const float vcl = v_old + fminf(fmaxf(dvo, -clip_range_vf), clip_range_vf);
    const float l2 = vf_loss(vf_fn, vcl - R);
    float w1, w2;
    if (l > l2) { w1 = gl; w2 = 0.f; }
    else if (l < l2) { w1 = 0.f; w2 = gl; }
    else { w1 = gl * 0.5f; w2 = gl * 0.5f; }
    const float inside = (dvo >= -clip_range_vf && dvo <= clip_range_vf) ? 1.f : 0.f;
    t.dv = w1 * vf_grad(vf_fn, v - R) + (w2 * vf_grad(vf_fn, vcl - R)) * inside;
    t.clipped = (fabsf(v - v_old) > clip_range_vf) ? 1.f : 0.f;
    t.loss = fmaxf(l, l2);
  } else {
    t.dv = gl * vf_grad(vf_fn, v - R);
    t.clipped = 0.f;
    t.loss = l;
  }
  return t;
}

#endif  // RAI_PPO_TERMS_H
