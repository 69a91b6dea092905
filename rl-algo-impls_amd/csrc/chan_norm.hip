// Channel layer norm of the squeeze-U-Net (config C5 with `normalization: layer`) on gfx950.
//
// ChannelLayerNorm2d (rl_algo_impls/shared/module/channel_layer_norm.py) normalises every pixel of an
// NCHW activation over its channels with the UNBIASED variance (x.var(dim=1): divides by C - 1) and
// eps = 1e-5, and sits after every convolution of the backbone and the critic heads, mostly followed
// by a GELU.  As a torch composition that is a bias pass, two reductions and five elementwise passes
// forward and about three times that backward.  Here, over NHWC rows (rows = B*H*W, C fastest), with
// x the bias-free convolution output:
//   forward   one pass:  z = x + bias[c];  mean, var = sum (z - mean)^2 / (C - 1)  (two-pass, from the
//             centred values in registers);  rstd = 1 / sqrt(var + eps);
//             y = gamma[c] * (z - mean) * rstd + beta[c];  out = gelu ? GELU(y) : y;  stats = (mean, rstd)
//   backward  two launches:  dy = dout * (gelu ? GELU'(y) : 1),  g = dy * gamma,  xh = (z - mean) * rstd
//             dx = rstd * (g - mean_c(g) - xh * sum_c(g * xh) / (C - 1))
//             dgamma[c] = sum_rows dy * xh,  dbeta[c] = sum_rows dy,  dbias[c] = sum_rows dx
//             (the C - 1: d rstd / d z_j = -rstd^3 (z_j - mean) / (C - 1) from the unbiased variance)
//
// Work split: a row is held by C/4 lanes, one float4 each, so 64 / (C/4) rows share a wave and the row
// sums are cross-lane reductions of that width (DPP quad / mirror steps, then v_permlane16_swap and
// v_permlane32_swap for C = 128 and 256): no LDS and no second read of the row.  The column sums:
// workgroup w owns a fixed run of rows and keeps three float4 accumulators per thread; its row lanes
// are tree-summed through LDS and the workgroup's sums go to partial[w]; a second launch sums the
// partials.  Every order is fixed by (rows, C), so the gradients are deterministic, and the kernel
// boundary is the only hand-off between workgroups (no counters, so the workspace needs no zeroing).
#include <algorithm>

#include "common.h"
#include "gelu.h"

namespace {

constexpr int CLN_THREADS = 256;
constexpr int CLN_MAX_BLOCKS = 1024;    // row-pass workgroups of the backward: four per CU
constexpr int CLN_ROWS_PER_LANE = 8;    // rows per row lane before another workgroup is added
constexpr int CLN_FWD_MAX_BLOCKS = 2048;
constexpr int CLN_FIN_C4 = 16;          // float4 channel groups per finalize workgroup
using f4 = float __attribute__((ext_vector_type(4)));

// bias / gamma / beta are views into the flat parameter buffer: 4-byte aligned only
__device__ __forceinline__ f4 ld_par4(const float* __restrict__ p, int c4) {
  return f4{p[4 * c4], p[4 * c4 + 1], p[4 * c4 + 2], p[4 * c4 + 3]};
}

// Sum over the L lanes (an aligned group, L in {4, 8, 16, 32, 64}) that hold one row; every lane of
// the group ends with the same bits.  The steps are wave_sum_dpp's (common.h), cut at the group's
// width.  All 64 lanes must be active.
template <int L>
__device__ __forceinline__ float group_sum(float v) {
  v += __int_as_float(rai_dpp<0xB1>(__float_as_int(v)));  // quad_perm [1,0,3,2]
  v += __int_as_float(rai_dpp<0x4E>(__float_as_int(v)));  // quad_perm [2,3,0,1]
  if constexpr (L >= 8) v += __int_as_float(rai_dpp<0x141>(__float_as_int(v)));   // row_half_mirror
  if constexpr (L >= 16) v += __int_as_float(rai_dpp<0x140>(__float_as_int(v)));  // row_mirror
  if constexpr (L >= 32) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
  if constexpr (L >= 64) {
    const auto q = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(q[0]) + __uint_as_float(q[1]);
  }
  return v;
}

__device__ __forceinline__ float sum4(f4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// Thread (row lane = tid / L, c4 = tid % L); a workgroup pass covers CLN_THREADS / L rows.  The trip
// count is uniform over the workgroup (every lane reaches the cross-lane sums); rows past the end
// compute on row `rows - 1` and store nothing.
template <int L>
__global__ __launch_bounds__(CLN_THREADS) void cln_fwd_kernel(const f4* __restrict__ x, const float* __restrict__ bias,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int64_t rows, float eps,
                                                              int gelu, f4* __restrict__ out,
                                                              float* __restrict__ stats) {
  constexpr int RPB = CLN_THREADS / L;
  constexpr float inv_c = 1.f / (4 * L), inv_cm1 = 1.f / (4 * L - 1);
  const int c4 = threadIdx.x % L, lane = threadIdx.x / L;
  const f4 bv = ld_par4(bias, c4), gv = ld_par4(gamma, c4), be = ld_par4(beta, c4);
  const int64_t passes = (rows + RPB - 1) / RPB;
  for (int64_t p = blockIdx.x; p < passes; p += gridDim.x) {
    const int64_t row = p * RPB + lane;
    const bool live = row < rows;
    const int64_t r = live ? row : rows - 1;
    f4 z = x[r * L + c4];
    z += bv;
    const float mean = group_sum<L>(sum4(z)) * inv_c;
    const f4 d = z - mean;
    const float var = group_sum<L>(sum4(d * d)) * inv_cm1;
    const float rstd = 1.f / sqrtf(var + eps);
    f4 y = gv * (d * rstd) + be;
    if (gelu) {
#pragma unroll
      for (int q = 0; q < 4; ++q) y[q] = gelu_f(y[q]);
    }
    if (live) {
      out[r * L + c4] = y;
      if (c4 == 0) {
        stats[2 * r] = mean;
        stats[2 * r + 1] = rstd;
      }
    }
  }
}

// part[q][lane * L + c4] (q = dgamma, dbeta, dbias; row lanes a power of two) -> part[q][c4]: a
// pairwise tree over the row lanes, the same order on every launch.
template <int L>
__device__ __forceinline__ void cln_lane_tree(f4 (*part)[CLN_THREADS], int lane) {
  constexpr int RPB = CLN_THREADS / L;
#pragma unroll
  for (int h = RPB / 2; h >= 1; h /= 2) {
    if (lane < h) {
#pragma unroll
      for (int q = 0; q < 3; ++q) part[q][threadIdx.x] += part[q][threadIdx.x + h * L];
    }
    __syncthreads();
  }
}

// Workgroup w owns rows [w * rows_per_block, (w + 1) * rows_per_block); partial: (gridDim.x, 3, C).
template <int L>
__global__ __launch_bounds__(CLN_THREADS) void cln_bwd_kernel(const f4* __restrict__ dout, const f4* __restrict__ x,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              const float* __restrict__ stats, int64_t rows,
                                                              int64_t rows_per_block, int gelu, f4* __restrict__ dx,
                                                              f4* __restrict__ partial) {
  constexpr int RPB = CLN_THREADS / L;
  constexpr float inv_c = 1.f / (4 * L), inv_cm1 = 1.f / (4 * L - 1);
  __shared__ f4 part[3][CLN_THREADS];
  const int tid = threadIdx.x, c4 = tid % L, lane = tid / L;
  const f4 bv = ld_par4(bias, c4), gv = ld_par4(gamma, c4), be = ld_par4(beta, c4);
  const int64_t r0 = blockIdx.x * rows_per_block;
  const int64_t r1 = min(rows, r0 + rows_per_block);
  f4 a_dg = f4{0.f, 0.f, 0.f, 0.f}, a_db = a_dg, a_dz = a_dg;
  for (int64_t rb = r0; rb < r1; rb += RPB) {  // uniform over the workgroup
    const int64_t row = rb + lane;
    const bool live = row < r1;
    const int64_t r = live ? row : r1 - 1;
    const f4 go = dout[r * L + c4];
    f4 z = x[r * L + c4];
    const float mean = stats[2 * r], rstd = stats[2 * r + 1];
    z += bv;
    const f4 xh = (z - mean) * rstd;
    f4 dy = go;
    if (gelu) {
      const f4 y = gv * xh + be;
#pragma unroll
      for (int q = 0; q < 4; ++q) dy[q] = go[q] * gelu_grad(y[q]);
    }
    const f4 g = dy * gv;
    const float s1 = group_sum<L>(sum4(g)) * inv_c;
    const float s2 = group_sum<L>(sum4(g * xh)) * inv_cm1;
    const f4 dz = (g - s1 - xh * s2) * rstd;
    if (live) {
      dx[r * L + c4] = dz;
      a_dg += dy * xh;
      a_db += dy;
      a_dz += dz;
    }
  }
  part[0][tid] = a_dg;
  part[1][tid] = a_db;
  part[2][tid] = a_dz;
  __syncthreads();
  cln_lane_tree<L>(part, lane);
  if (tid < 3 * L) {  // 3 * L <= 192 < CLN_THREADS
    const int q = tid / L, c = tid % L;
    partial[((int64_t)blockIdx.x * 3 + q) * L + c] = part[q][c];
  }
}

// Second launch: workgroup (q, j) sums quantity q's nb partials for the float4 channel groups
// [j * CLN_FIN_C4, ...): thread (lane, c) adds partials lane, lane + 16, ... in order, then the 16
// lanes are tree-summed through LDS.
__global__ __launch_bounds__(CLN_THREADS) void cln_finalize_kernel(const f4* __restrict__ partial, int nb, int L,
                                                                   float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta,
                                                                   float* __restrict__ dbias) {
  constexpr int LANES = CLN_THREADS / CLN_FIN_C4;
  __shared__ f4 part[CLN_THREADS];
  const int tid = threadIdx.x, c = tid % CLN_FIN_C4, lane = tid / CLN_FIN_C4;
  const int q = blockIdx.x, c4 = blockIdx.y * CLN_FIN_C4 + c;
  f4 s = f4{0.f, 0.f, 0.f, 0.f};
  if (c4 < L)
    for (int w = lane; w < nb; w += LANES) s += partial[((int64_t)w * 3 + q) * L + c4];
  part[tid] = s;
  __syncthreads();
#pragma unroll
  for (int h = LANES / 2; h >= 1; h /= 2) {
    if (lane < h) part[tid] += part[tid + h * CLN_FIN_C4];
    __syncthreads();
  }
  if (lane == 0 && c4 < L) {
    float* o = q == 0 ? dgamma : q == 1 ? dbeta : dbias;
    const f4 t = part[tid];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[4 * c4 + k] = t[k];
  }
}

bool cln_shape_ok(int64_t rows, int32_t C) {
  if (rows < 0 || C < 16 || C > RAI_CLN_MAX_C || C % 4) return false;
  const int C4 = C / 4;
  return (C4 & (C4 - 1)) == 0;
}

int64_t cln_bwd_blocks(int64_t rows, int C4, int64_t* rows_per_block) {
  const int64_t rpb_pass = CLN_THREADS / C4;
  int64_t blocks = (rows + CLN_ROWS_PER_LANE * rpb_pass - 1) / (CLN_ROWS_PER_LANE * rpb_pass);
  blocks = std::max<int64_t>(1, std::min<int64_t>(blocks, CLN_MAX_BLOCKS));
  const int64_t rpb = (rows + blocks - 1) / blocks;
  *rows_per_block = rpb;
  return (rows + rpb - 1) / rpb;
}

}  // namespace

extern "C" int64_t rai_chan_ln_workspace_bytes(int32_t C) {
  return (int64_t)CLN_MAX_BLOCKS * 3 * (C > 0 ? C : 0) * 4;  // per-workgroup (dgamma, dbeta, dbias) partials
}

#define CLN_DISPATCH(C4, CALL) \
  switch (C4) {                \
    case 4: CALL(4); break;    \
    case 8: CALL(8); break;    \
    case 16: CALL(16); break;  \
    case 32: CALL(32); break;  \
    default: CALL(64); break;  \
  }

extern "C" int rai_chan_ln_fwd(const float* x, const float* bias, const float* gamma, const float* beta, int64_t rows,
                               int32_t C, float eps, int32_t gelu, float* out, float* stats, void* stream) {
  if (!cln_shape_ok(rows, C)) return RAI_E_SHAPE;
  if (rows == 0) return RAI_OK;
  if (!x || !bias || !gamma || !beta || !out || !stats) return RAI_E_NULLPTR;
  if ((((uintptr_t)x | (uintptr_t)out) & 15) || ((uintptr_t)stats & 3)) return RAI_E_WORKSPACE;
  const int C4 = C / 4;
  const int64_t passes = (rows + CLN_THREADS / C4 - 1) / (CLN_THREADS / C4);
  const unsigned blocks = (unsigned)std::min<int64_t>(passes, CLN_FWD_MAX_BLOCKS);
  hipStream_t st = rai_stream(stream);
#define CLN_FWD(L_)                                                                                               \
  hipLaunchKernelGGL(cln_fwd_kernel<L_>, dim3(blocks), dim3(CLN_THREADS), 0, st, reinterpret_cast<const f4*>(x), \
                     bias, gamma, beta, rows, eps, gelu, reinterpret_cast<f4*>(out), stats)
  CLN_DISPATCH(C4, CLN_FWD)
#undef CLN_FWD
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_chan_ln_bwd(const float* dout, const float* x, const float* bias, const float* gamma,
                               const float* beta, const float* stats, int64_t rows, int32_t C, int32_t gelu, float* dx,
                               float* dgamma, float* dbeta, float* dbias, void* workspace, int64_t workspace_bytes,
                               void* stream) {
  if (!cln_shape_ok(rows, C)) return RAI_E_SHAPE;
  if (!dgamma || !dbeta || !dbias) return RAI_E_NULLPTR;
  hipStream_t st = rai_stream(stream);
  if (rows == 0) {
    for (float* p : {dgamma, dbeta, dbias}) {
      const hipError_t e = hipMemsetAsync(p, 0, (size_t)C * 4, st);
      if (e != hipSuccess) return (int)e;
    }
    return RAI_OK;
  }
  if (!dout || !x || !bias || !gamma || !beta || !stats || !dx || !workspace) return RAI_E_NULLPTR;
  if (workspace_bytes < rai_chan_ln_workspace_bytes(C) ||
      (((uintptr_t)workspace | (uintptr_t)dout | (uintptr_t)x | (uintptr_t)dx) & 15) || ((uintptr_t)stats & 3))
    return RAI_E_WORKSPACE;
  const int C4 = C / 4;
  int64_t rpb = 0;
  const unsigned blocks = (unsigned)cln_bwd_blocks(rows, C4, &rpb);
  f4* partial = static_cast<f4*>(workspace);
#define CLN_BWD(L_)                                                                                                  \
  hipLaunchKernelGGL(cln_bwd_kernel<L_>, dim3(blocks), dim3(CLN_THREADS), 0, st, reinterpret_cast<const f4*>(dout), \
                     reinterpret_cast<const f4*>(x), bias, gamma, beta, stats, rows, rpb, gelu,                      \
                     reinterpret_cast<f4*>(dx), partial)
  CLN_DISPATCH(C4, CLN_BWD)
#undef CLN_BWD
  RAI_LAUNCH_CHECK();
  hipLaunchKernelGGL(cln_finalize_kernel, dim3(3, (unsigned)((C4 + CLN_FIN_C4 - 1) / CLN_FIN_C4)), dim3(CLN_THREADS),
                     0, st, partial, (int)blocks, C4, dgamma, dbeta, dbias);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}
