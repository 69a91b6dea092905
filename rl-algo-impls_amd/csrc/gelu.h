// The exact (erf) GELU of torch.nn.GELU() and its derivative, shared by the squeeze-U-Net epilogues
// (se_block.hip, chan_norm.hip): gelu(t) = t * Phi(t), gelu'(t) = Phi(t) + t * phi(t).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float gelu_f(float t) { return 0.5f * t * (1.f + erff(t * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad(float t) {
  const float cdf = 0.5f * (1.f + erff(t * 0.70710678118654752f));
  const float pdf = expf(-0.5f * t * t) * 0.39894228040143268f;
  return cdf + t * pdf;
}
