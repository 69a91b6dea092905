// Squeeze-excitation gate of the DoubleCone backbone's SE blocks on gfx950.
//
// SqueezeExcitation.forward (rl_algo_impls/shared/policy/actor_critic_network/double_cone.py:43-47)
// computes the per-sample channel scale   s = sigmoid(W2 . GELU(W1 . mean_hw r))   as an
// AdaptiveAvgPool2d, two bias-free Linears, a GELU and a sigmoid: five small launches forward and about
// twice that backward, 14 times per network, six of them on the cone's 4x4 map where they are as large
// as the convolutions beside them.  Here, with r NHWC (B, HW, C), W1 (M, C), W2 (C, M), M = C / 16:
//   forward   one launch:  pooled[b] = sum_hw r[b] / HW;  hidden[b] = W1 pooled[b];
//             s[b] = sigmoid(W2 GELU(hidden[b]))           (pooled, hidden kept for the backward)
//   backward  two launches:  dz2 = ds s (1 - s);  da = W2^T dz2;  dh = da GELU'(hidden);
//             dpool = W1^T dh;  dr[b, p, :] += dpool / HW  (in place: dr already holds the SE
//             epilogue's g * s);  dW2 = sum_b dz2 (x) GELU(hidden),  dW1 = sum_b dh (x) pooled
//
// Work split: a workgroup owns whole samples and carries SEG_CHUNK of them through the matrix-vector
// products together, so that every weight element read serves the whole chunk (W1 and W2 are 64 KB
// each at C = 512: per-sample reads would outweigh r).  The reductions over HW, over C and over the
// workgroup's thread groups all run in orders fixed by the shape; the sums over C and over M accumulate in
// float64 (a few thousand multiply-adds per sample, nothing beside r's traffic: the pooled values of a
// sample with a large common offset cancel in W1 . pooled, and float32 partial sums lose bits there).
// Backward: workgroup w owns the
// samples [w * run, (w + 1) * run) (so the in-place add cannot race), adds its chunks' weight-gradient
// terms into its own workspace slot (2, M, C: dW1, then dW2 transposed, written by the first chunk and
// added to by the later ones, every element by the same thread), and a second launch sums the slots in
// a fixed order.  No float atomics and no arrival counters: the workspace needs no zeroing and two
// calls on the same inputs give the same bits.  W1 and W2 are views into the flat parameter buffer
// (4-byte aligned only) and are read as scalars.
#include <algorithm>

#include "common.h"
#include "gelu.h"

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_CHUNK = RAI_SEG_CHUNK;            // samples carried through the GEMVs together
constexpr int SEG_MAX_BLOCKS = RAI_SEG_MAX_BLOCKS;  // backward workgroups = workspace slots
constexpr int SEG_FIN_LANES = RAI_SEG_FIN_LANES;    // slots summed side by side in the finalize
constexpr int SEG_FIN_G4 = SEG_THREADS / SEG_FIN_LANES;  // float4 element groups per finalize workgroup
constexpr int SEG_MAX_C = 1024;
constexpr int SEG_MAX_M = 64;
constexpr int SEG_FWD_MAX_BLOCKS = 2048;
using f4 = float __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float sigmoid_f(float z) { return 1.f / (1.f + expf(-z)); }

// Workgroup pass p covers the samples [p * spw, (p + 1) * spw), spw <= SEG_CHUNK.
__global__ __launch_bounds__(SEG_THREADS) void se_gate_fwd_kernel(const f4* __restrict__ r, const float* __restrict__ w1,
                                                                  const float* __restrict__ w2, int64_t B, int C, int HW,
                                                                  int M, int spw, float* __restrict__ s,
                                                                  f4* __restrict__ pooled, float* __restrict__ hidden) {
  __shared__ f4 part[SEG_THREADS];
  __shared__ float mean_s[SEG_CHUNK][SEG_MAX_C];
  __shared__ double hpart[SEG_CHUNK][SEG_THREADS];
  __shared__ float act[SEG_CHUNK][SEG_MAX_M];
  const int tid = threadIdx.x, C4 = C / 4;
  const int c4 = tid % C4, row0 = tid / C4, rstep = SEG_THREADS / C4;
  const int L = SEG_THREADS / M, hm = tid / L, hj = tid % L;  // hidden: L lanes per output m
  const float hw = (float)HW;
  for (int64_t b0 = (int64_t)blockIdx.x * spw; b0 < B; b0 += (int64_t)gridDim.x * spw) {
    const int ns = (int)min((int64_t)spw, B - b0);
    // column means: thread (row0, c4) adds rows row0, row0 + rstep, ...; the row groups in order
    for (int q = 0; q < ns; ++q) {
      const f4* rs = r + (b0 + q) * (int64_t)HW * C4;
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      for (int h = row0; h < HW; h += rstep) acc += rs[(int64_t)h * C4 + c4];
      part[tid] = acc;
      __syncthreads();
      if (tid < C4) {
        f4 t = part[tid];
        for (int k = 1; k < rstep; ++k) t += part[tid + k * C4];
        t = t / hw;
        pooled[(b0 + q) * C4 + tid] = t;
#pragma unroll
        for (int k = 0; k < 4; ++k) mean_s[q][4 * tid + k] = t[k];
      }
      __syncthreads();
    }
    // hidden[m] = sum_c W1[m, c] mean[c]: lane hj of output hm takes c = hj, hj + L, ...
    double ha[SEG_CHUNK];
#pragma unroll
    for (int q = 0; q < SEG_CHUNK; ++q) ha[q] = 0.0;
    for (int c = hj; c < C; c += L) {
      const double w = w1[hm * C + c];
#pragma unroll
      for (int q = 0; q < SEG_CHUNK; ++q)
        if (q < ns) ha[q] += w * (double)mean_s[q][c];
    }
#pragma unroll
    for (int q = 0; q < SEG_CHUNK; ++q) hpart[q][tid] = ha[q];
    __syncthreads();
    if (tid < M) {
      for (int q = 0; q < ns; ++q) {
        double hd = hpart[q][tid * L];
        for (int k = 1; k < L; ++k) hd += hpart[q][tid * L + k];
        const float h = (float)hd;
        hidden[(b0 + q) * M + tid] = h;
        act[q][tid] = gelu_f(h);
      }
    }
    __syncthreads();
    // s[c] = sigmoid(sum_m W2[c, m] act[m]): a thread per channel
    for (int c = tid; c < C; c += SEG_THREADS) {
      double z[SEG_CHUNK];
#pragma unroll
      for (int q = 0; q < SEG_CHUNK; ++q) z[q] = 0.0;
      for (int m = 0; m < M; ++m) {
        const double w = w2[c * M + m];
#pragma unroll
        for (int q = 0; q < SEG_CHUNK; ++q)
          if (q < ns) z[q] += w * (double)act[q][m];
      }
#pragma unroll
      for (int q = 0; q < SEG_CHUNK; ++q)
        if (q < ns) s[(b0 + q) * C + c] = sigmoid_f((float)z[q]);
    }
    __syncthreads();  // mean_s, hpart and act are rewritten by the next pass
  }
}

// Workgroup w owns the samples [w * run, (w + 1) * run) and the slot partial[w] (2, M, C).
__global__ __launch_bounds__(SEG_THREADS) void se_gate_bwd_kernel(const float* __restrict__ ds, const float* __restrict__ s,
                                                                  const float* __restrict__ pooled,
                                                                  const float* __restrict__ hidden,
                                                                  const float* __restrict__ w1,
                                                                  const float* __restrict__ w2, int64_t B, int C, int HW,
                                                                  int M, int64_t run, f4* dr, float* partial) {
  __shared__ float dz_s[SEG_CHUNK][SEG_MAX_C];
  __shared__ float dp_s[SEG_CHUNK][SEG_MAX_C];
  __shared__ double red[SEG_CHUNK][SEG_THREADS];
  __shared__ float a_s[SEG_CHUNK][SEG_MAX_M];
  __shared__ float dh_s[SEG_CHUNK][SEG_MAX_M];
  const int tid = threadIdx.x, C4 = C / 4, MC = M * C;
  const int G = SEG_THREADS / M, am = tid % M, aj = tid / M;  // da: G thread groups per output m
  const int64_t b_begin = (int64_t)blockIdx.x * run, b_end = min(B, b_begin + run);
  float* slot = partial + (int64_t)blockIdx.x * 2 * MC;
  const float hw = (float)HW;
  bool first = true;
  for (int64_t b0 = b_begin; b0 < b_end; b0 += SEG_CHUNK) {
    const int ns = (int)min((int64_t)SEG_CHUNK, b_end - b0);
    for (int q = 0; q < ns; ++q) {
      for (int c = tid; c < C; c += SEG_THREADS) {
        const float sv = s[(b0 + q) * C + c];
        dz_s[q][c] = ds[(b0 + q) * C + c] * sv * (1.f - sv);
      }
      if (tid < M) a_s[q][tid] = gelu_f(hidden[(b0 + q) * M + tid]);
    }
    __syncthreads();
    // da[m] = sum_c W2[c, m] dz2[c]: thread (aj, am) takes c = aj, aj + G, ...; the groups in order
    double da[SEG_CHUNK];
#pragma unroll
    for (int q = 0; q < SEG_CHUNK; ++q) da[q] = 0.0;
    for (int c = aj; c < C; c += G) {
      const double w = w2[c * M + am];
#pragma unroll
      for (int q = 0; q < SEG_CHUNK; ++q)
        if (q < ns) da[q] += w * (double)dz_s[q][c];
    }
#pragma unroll
    for (int q = 0; q < SEG_CHUNK; ++q) red[q][tid] = da[q];
    __syncthreads();
    if (tid < M) {
      for (int q = 0; q < ns; ++q) {
        double t = red[q][tid];
        for (int k = 1; k < G; ++k) t += red[q][tid + k * M];
        dh_s[q][tid] = (float)t * gelu_grad(hidden[(b0 + q) * M + tid]);
      }
    }
    __syncthreads();
    // a thread per channel: dpool[c] = sum_m W1[m, c] dh[m], and this chunk's terms of dW1[m, c] and
    // dW2[c, m] (stored transposed, (M, C), so that the slot's stores are contiguous over the threads)
    for (int c = tid; c < C; c += SEG_THREADS) {
      double dp[SEG_CHUNK];
      float pl[SEG_CHUNK], dz[SEG_CHUNK];
#pragma unroll
      for (int q = 0; q < SEG_CHUNK; ++q) {
        dp[q] = 0.0;
        pl[q] = q < ns ? pooled[(b0 + q) * C + c] : 0.f;
        dz[q] = q < ns ? dz_s[q][c] : 0.f;
      }
      for (int m = 0; m < M; ++m) {
        const double w = w1[m * C + c];
        double g1 = 0.0, g2 = 0.0;
#pragma unroll
        for (int q = 0; q < SEG_CHUNK; ++q) {
          if (q < ns) {
            const double dh = dh_s[q][m];
            dp[q] += w * dh;
            g1 += dh * (double)pl[q];
            g2 += (double)dz[q] * (double)a_s[q][m];
          }
        }
        const int i = m * C + c;
        slot[i] = first ? (float)g1 : slot[i] + (float)g1;
        slot[MC + i] = first ? (float)g2 : slot[MC + i] + (float)g2;
      }
#pragma unroll
      for (int q = 0; q < SEG_CHUNK; ++q)
        if (q < ns) dp_s[q][c] = (float)(dp[q] / (double)hw);
    }
    __syncthreads();
    // dr[b, p, :] += dpool / HW (C4 divides the workgroup size: a thread keeps its channel group)
    const int c4 = tid % C4;
    for (int q = 0; q < ns; ++q) {
      const f4 add = f4{dp_s[q][4 * c4], dp_s[q][4 * c4 + 1], dp_s[q][4 * c4 + 2], dp_s[q][4 * c4 + 3]};
      f4* drs = dr + (b0 + q) * (int64_t)HW * C4;
      for (int i = tid; i < HW * C4; i += SEG_THREADS) drs[i] += add;
    }
    __syncthreads();  // dz_s, dp_s, a_s, dh_s are rewritten by the next chunk
    first = false;
  }
}

// Second launch: thread (lane, g) adds float4 group g of the slots lane, lane + SEG_FIN_LANES, ... in
// order, the lanes are tree-summed through LDS, and dW1 (M, C) / dW2 (C, M) are written as scalars.
__global__ __launch_bounds__(SEG_THREADS) void se_gate_finalize_kernel(const f4* __restrict__ partial, int nb, int C,
                                                                       int M, float* __restrict__ dw1,
                                                                       float* __restrict__ dw2) {
  __shared__ f4 part[SEG_THREADS];
  const int tid = threadIdx.x, gi = tid % SEG_FIN_G4, lane = tid / SEG_FIN_G4;
  const int MC = M * C, total = 2 * MC / 4;  // float4 groups per slot
  const int g = blockIdx.x * SEG_FIN_G4 + gi;
  f4 t = f4{0.f, 0.f, 0.f, 0.f};
  if (g < total)
    for (int w = lane; w < nb; w += SEG_FIN_LANES) t += partial[(int64_t)w * total + g];
  part[tid] = t;
  __syncthreads();
#pragma unroll
  for (int h = SEG_FIN_LANES / 2; h >= 1; h /= 2) {
    if (lane < h) part[tid] += part[tid + h * SEG_FIN_G4];
    __syncthreads();
  }
  if (lane == 0 && g < total) {
    const f4 v = part[tid];
    const int e = 4 * g;  // MC % 4 == 0: a group lies in one matrix, and in one row m of it
    if (e < MC) {
#pragma unroll
      for (int k = 0; k < 4; ++k) dw1[e + k] = v[k];
    } else {
      const int i = e - MC, m = i / C, c = i % C;
#pragma unroll
      for (int k = 0; k < 4; ++k) dw2[(c + k) * M + m] = v[k];
    }
  }
}

bool seg_shape_ok(int64_t B, int32_t C, int32_t HW, int32_t M) {
  if (B < 0 || C < 16 || C > SEG_MAX_C || C % 16 || HW < 1) return false;
  const int C4 = C / 4;
  return SEG_THREADS % C4 == 0 && M == C / 16 && M <= SEG_MAX_M;  // M a power of two: divides 256
}

}  // namespace

extern "C" int64_t rai_se_gate_workspace_bytes(int32_t C) {
  const int64_t c = C > 0 ? C : 0;
  return (int64_t)SEG_MAX_BLOCKS * 2 * (c / 16) * c * 4;  // per-workgroup (dW1, dW2^T) slots
}

extern "C" int rai_se_gate_fwd(const float* r, const float* w1, const float* w2, int64_t B, int32_t C, int32_t HW,
                               int32_t M, float* s, float* pooled, float* hidden, void* stream) {
  if (!seg_shape_ok(B, C, HW, M)) return RAI_E_SHAPE;
  if (B == 0) return RAI_OK;
  if (!r || !w1 || !w2 || !s || !pooled || !hidden) return RAI_E_NULLPTR;
  if ((((uintptr_t)r | (uintptr_t)pooled) & 15) || (((uintptr_t)s | (uintptr_t)hidden) & 3)) return RAI_E_WORKSPACE;
  // the weights outweigh a sample's activations (2 M C against HW C floats): share them over a chunk
  const int spw = (2 * M >= HW && B >= 2 * SEG_CHUNK) ? SEG_CHUNK : 1;
  const unsigned blocks = (unsigned)std::min<int64_t>((B + spw - 1) / spw, SEG_FWD_MAX_BLOCKS);
  hipLaunchKernelGGL(se_gate_fwd_kernel, dim3(blocks), dim3(SEG_THREADS), 0, rai_stream(stream),
                     reinterpret_cast<const f4*>(r), w1, w2, B, C, HW, M, spw, s, reinterpret_cast<f4*>(pooled), hidden);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_se_gate_bwd(const float* ds, const float* s, const float* pooled, const float* hidden,
                               const float* w1, const float* w2, int64_t B, int32_t C, int32_t HW, int32_t M, float* dr,
                               float* dw1, float* dw2, void* workspace, int64_t workspace_bytes, void* stream) {
  if (!seg_shape_ok(B, C, HW, M)) return RAI_E_SHAPE;
  if (!dw1 || !dw2) return RAI_E_NULLPTR;
  hipStream_t st = rai_stream(stream);
  if (B == 0) {
    for (float* p : {dw1, dw2}) {
      const hipError_t e = hipMemsetAsync(p, 0, (size_t)M * C * 4, st);
      if (e != hipSuccess) return (int)e;
    }
    return RAI_OK;
  }
  if (!ds || !s || !pooled || !hidden || !w1 || !w2 || !dr || !workspace) return RAI_E_NULLPTR;
  if (workspace_bytes < rai_se_gate_workspace_bytes(C) || (((uintptr_t)workspace | (uintptr_t)dr) & 15))
    return RAI_E_WORKSPACE;
  const int64_t run = (B + SEG_MAX_BLOCKS - 1) / SEG_MAX_BLOCKS;
  const unsigned blocks = (unsigned)((B + run - 1) / run);  // <= SEG_MAX_BLOCKS
  float* partial = static_cast<float*>(workspace);
  hipLaunchKernelGGL(se_gate_bwd_kernel, dim3(blocks), dim3(SEG_THREADS), 0, st, ds, s, pooled, hidden, w1, w2, B, C,
                     HW, M, run, reinterpret_cast<f4*>(dr), partial);
  RAI_LAUNCH_CHECK();
  const int total = 2 * M * C / 4;
  hipLaunchKernelGGL(se_gate_finalize_kernel, dim3((unsigned)((total + SEG_FIN_G4 - 1) / SEG_FIN_G4)),
                     dim3(SEG_THREADS), 0, st, reinterpret_cast<const f4*>(partial), (int)blocks, C, M, dw1, dw2);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

// ---- the cone's last up-convolution: out = skip + GELU(x + b[c]) --------------------------------
// DoubleConeBlock.forward (double_cone.py:130-131) adds the block's input to the GELU of the second
// transposed convolution; the bias + GELU pass and the add become one pass.  Backward: dskip = dout,
// dx = rai_bias_gelu_bwd.
namespace {
__global__ __launch_bounds__(SEG_THREADS) void bias_gelu_add_fwd_kernel(const f4* __restrict__ x,
                                                                        const float* __restrict__ b,
                                                                        const f4* __restrict__ skip, int C4, int64_t n4,
                                                                        f4* __restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)SEG_THREADS + threadIdx.x; i < n4; i += (int64_t)gridDim.x * SEG_THREADS) {
    const int c4 = (int)(i % C4);
    const f4 xv = x[i], kv = skip[i];
    const f4 bv = f4{b[4 * c4], b[4 * c4 + 1], b[4 * c4 + 2], b[4 * c4 + 3]};
    f4 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // GELU(t) is -0 for t < ~-5.6 (1 + erf = 0) and +0 + -0 = +0: a zero skip passes the GELU's own bits
      // through, so that a skip of zeros is rai_bias_gelu_fwd bit for bit
      const float g = gelu_f(xv[q] + bv[q]);
      o[q] = kv[q] == 0.f ? g : kv[q] + g;
    }
    out[i] = o;
  }
}
}  // namespace

extern "C" int rai_bias_gelu_add_fwd(const float* x, const float* b, const float* skip, int64_t rows, int32_t C,
                                     float* out, void* stream) {
  if (rows < 0 || C < 4 || C % 4) return RAI_E_SHAPE;
  if (rows == 0) return RAI_OK;
  if (!x || !b || !skip || !out) return RAI_E_NULLPTR;
  const int64_t n4 = rows * (C / 4);
  const int64_t blocks = std::min<int64_t>((n4 + SEG_THREADS - 1) / SEG_THREADS, 256 * 64);
  hipLaunchKernelGGL(bias_gelu_add_fwd_kernel, dim3((unsigned)blocks), dim3(SEG_THREADS), 0, rai_stream(stream),
                     reinterpret_cast<const f4*>(x), b, reinterpret_cast<const f4*>(skip), C / 4, n4,
                     reinterpret_cast<f4*>(out));
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}
