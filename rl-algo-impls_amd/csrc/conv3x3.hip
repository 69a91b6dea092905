// IMPALA CNN layers (cnn_style: impala) as hand-written f32 MFMA kernels on gfx950.
//
// Reference: rl_algo_impls/shared/encoder/impala_cnn.py:11-92 -- per ConvSequence one Conv2d(3x3, pad 1),
// MaxPool2d(3, stride 2, pad 1) and two pre-activation residual blocks x + conv(relu(conv(relu(x)))),
// then one final activation.  Every convolution is 3x3 / stride 1 / pad 1, so output pixel p reads the
// input pixels p + (dh, dw), dh, dw in {-1, 0, 1}; a tap that falls outside the image is a zero
// (predicated loads: no padded copy exists anywhere).
//
// Layouts as csrc/conv.hip: activations NHWC fp32, weights channels_last [Co][3][3][Ci], bias [Co].
//
// GEMM view of the forward: y^T[co][p] = sum over (tap, ci) of w[co][tap][ci] * pre(x)[p + tap][ci].
// v_mfma_f32_16x16x4f32 takes lane (i, g) = (lane % 16, lane / 16) as row i of A and column i of B at
// reduction index g, and returns rows 4g .. 4g+3 of column i.  Rows are output channels, columns are
// pixels: per tap and per 16 input channels, lane group g loads channels 16q + 4g .. +3 of its weight
// row and of its pixel as one float4 each, and four MFMAs take component j of both.  A lane ends with
// four consecutive output channels of one pixel: one float4 of the NHWC row, where the epilogue (bias,
// mask, residual, ReLU) is applied.
//
// Tile choice.  A wave always owns four 16x16 output blocks (16 accumulator VGPRs), arranged by the
// channel count: Co % 64 == 0 -> 4 channel tiles x 1 pixel tile, Co % 32 == 0 -> 2 x 2, else (Co = 16,
// the first procgen sequence) 1 x 4.  With Co = 16 there is a single weight tile, so the only operand
// reuse available is across pixels: one float4 of weights feeds four pixel tiles (16 MFMAs per 5
// float4 loads, against 4 per 2 for a 1 x 1 wave).
//
// The input gradient is the same kernel (template DG): dx[p][ci] = sum over (tap, co) of
// dz[p + tap][co] * w[co][8 - tap][ci], i.e. the forward over dz with the roles of Ci and Co swapped
// and the weight read through a transposed index (four strided scalar loads per lane instead of one
// float4; consecutive lanes read consecutive ci).  No transposed weight copy is made.
//
// Everything is deterministic: no atomics, fixed summation order.
#include "common.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int C3_THREADS = 256;
constexpr int C3_MAX_SPLITS = 512;

struct C3Args {
  const float* x;    // forward: the input (B, H, W, CK); input gradient: dz (B, H, W, CK)
  const float* w;    // (Co, 3, 3, Ci)
  const float* b;    // [CN] or nullptr
  const float* m;    // (B, H, W, CN) or nullptr: outputs where m <= 0 are zeroed (threshold_backward)
  const float* res;  // (B, H, W, CN) or nullptr: added after the mask
  float* y;          // (B, H, W, CN), or (B, CN * H * W) with nchw
  int64_t M;         // B * H * W
  int H, W, CK, CN;  // CK: reduction channels, CN: output channels
  int pre, post, nchw;
};

__device__ __forceinline__ float relu_keep_nan(float t) { return t < 0.f ? 0.f : t; }

template <int NT, int TPX, bool DG>
__global__ __launch_bounds__(C3_THREADS) void conv3x3_kernel(const C3Args a) {
  static_assert(NT * TPX == 4, "four output blocks per wave");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int64_t px0 = (int64_t)blockIdx.x * (64 * TPX) + (int64_t)wv * (16 * TPX);
  const int c0 = blockIdx.y * (16 * NT);
  const int HW = a.H * a.W;

  const float* xb[TPX];
  int ph[TPX], pw[TPX];
  bool pv[TPX];
#pragma unroll
  for (int tp = 0; tp < TPX; ++tp) {
    int64_t p = px0 + 16 * tp + li;
    pv[tp] = p < a.M;
    p = pv[tp] ? p : a.M - 1;
    const int64_t n = p / HW;
    const int r = (int)(p - n * HW);
    ph[tp] = r / a.W;
    pw[tp] = r - ph[tp] * a.W;
    xb[tp] = a.x + p * a.CK;
  }

  f4 acc[NT][TPX];
#pragma unroll
  for (int tc = 0; tc < NT; ++tc)
#pragma unroll
    for (int tp = 0; tp < TPX; ++tp) acc[tc][tp] = f4{0.f, 0.f, 0.f, 0.f};

  const int nq = a.CK >> 4;
  for (int t = 0; t < 9; ++t) {
    const int dh = t / 3 - 1, dw = t - (t / 3) * 3 - 1;
    const int tw = DG ? 8 - t : t;
    const float* xp[TPX];
    bool ok[TPX];
#pragma unroll
    for (int tp = 0; tp < TPX; ++tp) {
      const int h = ph[tp] + dh, w = pw[tp] + dw;
      ok[tp] = pv[tp] && h >= 0 && h < a.H && w >= 0 && w < a.W;
      xp[tp] = xb[tp] + (int64_t)(dh * a.W + dw) * a.CK;
    }
    for (int q = 0; q < nq; ++q) {
      const int kk = 16 * q + 4 * g;
      f4 A[NT], Bv[TPX];
#pragma unroll
      for (int tc = 0; tc < NT; ++tc) {
        const int r = c0 + 16 * tc + li;
        if (!DG) {
          A[tc] = *reinterpret_cast<const f4*>(a.w + ((int64_t)r * 9 + tw) * a.CK + kk);
        } else {
          const float* wp = a.w + ((int64_t)kk * 9 + tw) * a.CN + r;
          const int64_t ks = (int64_t)9 * a.CN;
          A[tc] = f4{wp[0], wp[ks], wp[2 * ks], wp[3 * ks]};
        }
      }
#pragma unroll
      for (int tp = 0; tp < TPX; ++tp) {
        f4 v = f4{0.f, 0.f, 0.f, 0.f};
        if (ok[tp]) v = *reinterpret_cast<const f4*>(xp[tp] + kk);
        if (a.pre) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = relu_keep_nan(v[j]);
        }
        Bv[tp] = v;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int tc = 0; tc < NT; ++tc)
#pragma unroll
          for (int tp = 0; tp < TPX; ++tp)
            acc[tc][tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[tc][j], Bv[tp][j], acc[tc][tp], 0, 0, 0);
    }
  }

#pragma unroll
  for (int tc = 0; tc < NT; ++tc) {
    const int c = c0 + 16 * tc + 4 * g;
    f4 bv = f4{0.f, 0.f, 0.f, 0.f};
    if (a.b) bv = *reinterpret_cast<const f4*>(a.b + c);
#pragma unroll
    for (int tp = 0; tp < TPX; ++tp) {
      const int64_t p = px0 + 16 * tp + li;
      if (p >= a.M) continue;
      f4 v = acc[tc][tp] + bv;
      if (a.m) {
        const f4 mv = *reinterpret_cast<const f4*>(a.m + p * a.CN + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = mv[r] <= 0.f ? 0.f : v[r];
      }
      if (a.res) v += *reinterpret_cast<const f4*>(a.res + p * a.CN + c);
      if (a.post) {
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = relu_keep_nan(v[r]);
      }
      if (!a.nchw) {
        *reinterpret_cast<f4*>(a.y + p * a.CN + c) = v;
      } else {
        const int64_t n = p / HW;
        float* yb = a.y + n * (int64_t)a.CN * HW + (p - n * HW) + (int64_t)c * HW;
#pragma unroll
        for (int r = 0; r < 4; ++r) yb[(int64_t)r * HW] = v[r];
      }
    }
  }
}

// ---- first layer: Ci 3 or 4, uint8 (x / xdiv, IEEE division) or fp32 input ----------------------------
// K = 9 * Ci = 27 or 36 reduction elements in (tap, ci) order, walked four at a time: lane group g of
// step s holds element 4s + g.  27 is no multiple of 4: the last step's element 27 is a zero weight and
// a zero input in registers (nothing is padded in memory).  One channel tile x four pixel tiles per
// wave; the wave's <= 9 weight values stay in registers.
struct C3FirstArgs {
  const void* x;
  float xdiv;
  const float* w;
  const float* b;
  float* y;
  int64_t M;
  int H, W, Ci, Co;
};

template <bool U8>
__device__ __forceinline__ float first_load(const void* x, int64_t idx, float xdiv) {
  if (U8) return (float)reinterpret_cast<const uint8_t*>(x)[idx] / xdiv;
  return reinterpret_cast<const float*>(x)[idx];
}

template <bool U8>
__global__ __launch_bounds__(C3_THREADS) void conv3x3_first_kernel(const C3FirstArgs a) {
  constexpr int TPX = 4;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int64_t px0 = (int64_t)blockIdx.x * (64 * TPX) + (int64_t)wv * (16 * TPX);
  const int c0 = blockIdx.y * 16;
  const int HW = a.H * a.W, K = 9 * a.Ci, NS = (K + 3) >> 2;

  int64_t pb[TPX];
  int ph[TPX], pw[TPX];
  bool pv[TPX];
#pragma unroll
  for (int tp = 0; tp < TPX; ++tp) {
    int64_t p = px0 + 16 * tp + li;
    pv[tp] = p < a.M;
    p = pv[tp] ? p : a.M - 1;
    const int64_t n = p / HW;
    const int r = (int)(p - n * HW);
    ph[tp] = r / a.W;
    pw[tp] = r - ph[tp] * a.W;
    pb[tp] = p;
  }
  f4 acc[TPX];
#pragma unroll
  for (int tp = 0; tp < TPX; ++tp) acc[tp] = f4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int s = 0; s < 9; ++s) {
    if (s < NS) {
      const int k = 4 * s + g;
      const bool kv = k < K;
      const int kc = kv ? k : 0;
      const int tap = kc / a.Ci, ci = kc - tap * a.Ci;
      const int dh = tap / 3 - 1, dw = tap - (tap / 3) * 3 - 1;
      const float A = kv ? a.w[(int64_t)(c0 + li) * K + kc] : 0.f;
#pragma unroll
      for (int tp = 0; tp < TPX; ++tp) {
        const int h = ph[tp] + dh, w = pw[tp] + dw;
        float v = 0.f;
        if (kv && pv[tp] && h >= 0 && h < a.H && w >= 0 && w < a.W)
          v = first_load<U8>(a.x, (pb[tp] + dh * a.W + dw) * a.Ci + ci, a.xdiv);
        acc[tp] = __builtin_amdgcn_mfma_f32_16x16x4f32(A, v, acc[tp], 0, 0, 0);
      }
    }
  }
  const int c = c0 + 4 * g;
  const f4 bv = *reinterpret_cast<const f4*>(a.b + c);
#pragma unroll
  for (int tp = 0; tp < TPX; ++tp) {
    const int64_t p = px0 + 16 * tp + li;
    if (p >= a.M) continue;
    *reinterpret_cast<f4*>(a.y + p * a.Co + c) = acc[tp] + bv;
  }
}

// ---- MaxPool2d(3, stride 2, padding 1) ----------------------------------------------------------------
// One thread per output pixel and four channels.  As torch's CPU kernel: the running maximum starts at
// -inf with the first in-bounds window position as its index, and a later position replaces it when its
// value is greater or NaN (so the first of equal values wins and a NaN propagates).  argmax holds the
// window position kh * 3 + kw.
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, int64_t n4, int H, int W, int C,
                                                          int OH, int OW, float* __restrict__ y,
                                                          uint8_t* __restrict__ am) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int C4 = C >> 2;
  const int c = (int)(i % C4) * 4;
  const int64_t op = i / C4;
  const int ow = (int)(op % OW);
  const int64_t t = op / OW;
  const int oh = (int)(t % OH);
  const int64_t n = t / OH;
  f4 best = f4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  int idx[4];
  bool first = true;
  for (int kh = 0; kh < 3; ++kh) {
    const int h = 2 * oh - 1 + kh;
    if (h < 0 || h >= H) continue;
    for (int kw = 0; kw < 3; ++kw) {
      const int w = 2 * ow - 1 + kw;
      if (w < 0 || w >= W) continue;
      const f4 v = *reinterpret_cast<const f4*>(x + ((n * H + h) * W + w) * C + c);
      const int k = kh * 3 + kw;
      if (first) {
#pragma unroll
        for (int r = 0; r < 4; ++r) idx[r] = k;
        first = false;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (v[r] > best[r] || v[r] != v[r]) {
          best[r] = v[r];
          idx[r] = k;
        }
      }
    }
  }
  *reinterpret_cast<f4*>(y + op * C + c) = best;
  *reinterpret_cast<uint32_t*>(am + op * C + c) =
      (uint32_t)idx[0] | ((uint32_t)idx[1] << 8) | ((uint32_t)idx[2] << 16) | ((uint32_t)idx[3] << 24);
}

// Gather form of the backward: one thread per input pixel and four channels sums dy of the (at most
// 2 x 2) windows that contain the pixel and whose argmax names it, in (oh, ow) order.  Every dx element
// is written.
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dy,
                                                          const uint8_t* __restrict__ am, int64_t n4, int H, int W,
                                                          int C, int OH, int OW, float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int C4 = C >> 2;
  const int c = (int)(i % C4) * 4;
  const int64_t ip = i / C4;
  const int w = (int)(ip % W);
  const int64_t t = ip / W;
  const int h = (int)(t % H);
  const int64_t n = t / H;
  f4 s = f4{0.f, 0.f, 0.f, 0.f};
  const int oh0 = h >> 1, oh1 = (h + 1) >> 1, ow0 = w >> 1, ow1 = (w + 1) >> 1;
  for (int oh = oh0; oh <= oh1; ++oh) {
    if (oh >= OH) continue;
    const int kh = h - (2 * oh - 1);
    for (int ow = ow0; ow <= ow1; ++ow) {
      if (ow >= OW) continue;
      const int kw = w - (2 * ow - 1);
      const uint32_t k = (uint32_t)(kh * 3 + kw);
      const int64_t o = ((n * OH + oh) * OW + ow) * C + c;
      const uint32_t a4 = *reinterpret_cast<const uint32_t*>(am + o);
      const f4 g = *reinterpret_cast<const f4*>(dy + o);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (((a4 >> (8 * r)) & 255u) == k) s[r] += g[r];
    }
  }
  *reinterpret_cast<f4*>(dx + ip * C + c) = s;
}

// ---- weight gradient ----------------------------------------------------------------------------------
// dw[co][tap][ci] = sum_p dz[p][co] * pre(x)[p + tap][ci], db[co] = sum_p dz[p][co].  MFMA rows are
// output channels, columns input channels, the reduction runs over pixels four at a time (lane group g
// holds pixel p4 + g).  A wave owns one (16 co x 16 ci) pair for all nine taps (nine accumulators) over
// one contiguous split of the pixels and writes its tile to the workspace [split][Co][9][Ci]; the bias
// partials [split][Co] follow.  A second launch adds the splits in order.
struct C3WrwArgs {
  const void* x;
  float xdiv;
  const float* dz;
  float* part;
  int64_t M, chunk;  // pixels per split (a multiple of 4)
  int H, W, Ci, Co, S, pre;
};

__global__ __launch_bounds__(C3_THREADS) void conv3x3_wrw_kernel(const C3WrwArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int s = blockIdx.x * 4 + wv;
  const int nci = a.Ci >> 4;
  const int tco = blockIdx.y / nci, tci = blockIdx.y - tco * nci;
  const int co0 = 16 * tco, ci0 = 16 * tci;
  const int HW = a.H * a.W;
  const float* x = reinterpret_cast<const float*>(a.x);
  const int64_t beg = (int64_t)s * a.chunk;
  int64_t end = beg + a.chunk;
  end = end < a.M ? end : a.M;

  f4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = f4{0.f, 0.f, 0.f, 0.f};
  float dbl = 0.f;
  for (int64_t p4 = beg; p4 < end; p4 += 4) {
    const int64_t p = p4 + g;
    const bool pv = p < end;
    const int64_t pc = pv ? p : beg;
    const float dv = pv ? a.dz[pc * a.Co + co0 + li] : 0.f;
    dbl += dv;
    const int64_t n = pc / HW;
    const int r = (int)(pc - n * HW);
    const int h = r / a.W, w = r - h * a.W;
    const float* xp = x + pc * a.Ci + ci0 + li;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int dh = t / 3 - 1, dw = t % 3 - 1;
      const int hh = h + dh, ww = w + dw;
      float v = 0.f;
      if (pv && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W) v = xp[(int64_t)(dh * a.W + dw) * a.Ci];
      if (a.pre) v = relu_keep_nan(v);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, v, acc[t], 0, 0, 0);
    }
  }
  const int64_t KK = (int64_t)9 * a.Ci;
  float* out = a.part + (int64_t)s * a.Co * KK;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[(int64_t)(co0 + 4 * g + r) * KK + t * a.Ci + ci0 + li] = acc[t][r];
  if (tci == 0) {  // the bias partial: pixels g, g + 4, ... of this lane, then the four lane groups in order
    const float s0 = __shfl(dbl, li, 64), s1 = __shfl(dbl, li + 16, 64), s2 = __shfl(dbl, li + 32, 64),
                s3 = __shfl(dbl, li + 48, 64);
    if (g == 0) a.part[(int64_t)a.S * a.Co * KK + (int64_t)s * a.Co + co0 + li] = ((s0 + s1) + s2) + s3;
  }
}

// First layer: the columns are the K = 9 * Ci (tap, ci) elements themselves, in up to three tiles of 16
// (27 -> 2, 36 -> 3); columns >= K are zeros in registers and are not stored.
template <bool U8>
__global__ __launch_bounds__(C3_THREADS) void conv3x3_wrw_first_kernel(const C3WrwArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int s = blockIdx.x * 4 + wv;
  const int co0 = 16 * blockIdx.y;
  const int HW = a.H * a.W, K = 9 * a.Ci, NKT = (K + 15) >> 4;
  const int64_t beg = (int64_t)s * a.chunk;
  int64_t end = beg + a.chunk;
  end = end < a.M ? end : a.M;

  int kdh[3], kdw[3], koff[3];
  bool kv[3];
#pragma unroll
  for (int kt = 0; kt < 3; ++kt) {
    const int k = 16 * kt + li;
    kv[kt] = kt < NKT && k < K;
    const int kc = kv[kt] ? k : 0;
    const int tap = kc / a.Ci, ci = kc - tap * a.Ci;
    kdh[kt] = tap / 3 - 1;
    kdw[kt] = tap - (tap / 3) * 3 - 1;
    koff[kt] = (kdh[kt] * a.W + kdw[kt]) * a.Ci + ci;
  }
  f4 acc[3];
#pragma unroll
  for (int kt = 0; kt < 3; ++kt) acc[kt] = f4{0.f, 0.f, 0.f, 0.f};
  float dbl = 0.f;
  for (int64_t p4 = beg; p4 < end; p4 += 4) {
    const int64_t p = p4 + g;
    const bool pv = p < end;
    const int64_t pc = pv ? p : beg;
    const float dv = pv ? a.dz[pc * a.Co + co0 + li] : 0.f;
    dbl += dv;
    const int64_t n = pc / HW;
    const int r = (int)(pc - n * HW);
    const int h = r / a.W, w = r - h * a.W;
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) {
      if (kt < NKT) {
        const int hh = h + kdh[kt], ww = w + kdw[kt];
        float v = 0.f;
        if (pv && kv[kt] && hh >= 0 && hh < a.H && ww >= 0 && ww < a.W)
          v = first_load<U8>(a.x, pc * a.Ci + koff[kt], a.xdiv);
        acc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, v, acc[kt], 0, 0, 0);
      }
    }
  }
  float* out = a.part + (int64_t)s * a.Co * K;
#pragma unroll
  for (int kt = 0; kt < 3; ++kt)
    if (kv[kt]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(int64_t)(co0 + 4 * g + r) * K + 16 * kt + li] = acc[kt][r];
    }
  const float s0 = __shfl(dbl, li, 64), s1 = __shfl(dbl, li + 16, 64), s2 = __shfl(dbl, li + 32, 64),
              s3 = __shfl(dbl, li + 48, 64);
  if (g == 0) a.part[(int64_t)a.S * a.Co * K + (int64_t)s * a.Co + co0 + li] = ((s0 + s1) + s2) + s3;
}

// Sum of the S splits in order (element i of dw, then of db), stored or added.
__global__ __launch_bounds__(256) void conv3x3_wrw_reduce_kernel(const float* __restrict__ part, int S, int64_t nw,
                                                                 int Co, float* __restrict__ dw,
                                                                 float* __restrict__ db, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nw + Co) return;
  const bool bias = i >= nw;
  if (bias && !db) return;
  const float* src = bias ? part + (int64_t)S * nw + (i - nw) : part + i;
  const int64_t stride = bias ? Co : nw;
  float sum = 0.f;
  for (int s = 0; s < S; ++s) sum += src[(int64_t)s * stride];
  float* dst = bias ? db + (i - nw) : dw + i;
  *dst = accumulate ? *dst + sum : sum;
}

// ---- host ---------------------------------------------------------------------------------------------
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool chan_ok(int32_t c) { return c >= 16 && c <= 128 && c % 16 == 0; }

// Splits of the pixel range for the weight gradient: enough waves for 256 CUs x 8 over the layer's
// tile pairs, at least 64 pixels per wave, a multiple of the four waves of a workgroup.
int wrw_splits(int64_t M, int pairs) {
  int64_t want = (2048 + pairs - 1) / pairs;
  const int64_t cap = (M + 63) / 64;
  want = want < cap ? want : cap;
  want = want < 1 ? 1 : want;
  want = want > C3_MAX_SPLITS ? C3_MAX_SPLITS : want;
  return (int)((want + 3) / 4 * 4);
}

int wrw_pairs(int32_t Ci, int32_t Co) { return Ci <= 4 ? Co / 16 : (Co / 16) * (Ci / 16); }

int launch_conv(const C3Args& a, bool dg, hipStream_t st) {
  if (a.M == 0) return RAI_OK;
  const int nt = a.CN % 64 == 0 ? 4 : (a.CN % 32 == 0 ? 2 : 1);
  const int tpx = 4 / nt;
  const int64_t gx = (a.M + 64 * tpx - 1) / (64 * tpx);
  if (gx > 0x7fffffffLL) return RAI_E_SHAPE;
  const dim3 grid((unsigned)gx, (unsigned)(a.CN / (16 * nt)));
#define C3_LAUNCH(NT, TPX)                                                                    \
  do {                                                                                        \
    if (dg)                                                                                   \
      hipLaunchKernelGGL((conv3x3_kernel<NT, TPX, true>), grid, dim3(C3_THREADS), 0, st, a);  \
    else                                                                                      \
      hipLaunchKernelGGL((conv3x3_kernel<NT, TPX, false>), grid, dim3(C3_THREADS), 0, st, a); \
  } while (0)
  if (nt == 4) C3_LAUNCH(4, 1);
  else if (nt == 2) C3_LAUNCH(2, 2);
  else C3_LAUNCH(1, 4);
#undef C3_LAUNCH
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

int wrw_common(const void* x, bool first, bool u8, float xdiv, const float* dz, int64_t B, int32_t H, int32_t W,
               int32_t Ci, int32_t Co, int32_t pre, float* dw, float* db, int32_t accumulate, void* ws,
               int64_t ws_bytes, hipStream_t st) {
  if (!x || !dz || !dw || !ws) return RAI_E_NULLPTR;
  if (B < 0 || H < 1 || W < 1) return RAI_E_SHAPE;
  if (!chan_ok(Co) || (first ? (Ci != 3 && Ci != 4) : !chan_ok(Ci))) return RAI_E_UNSUPPORTED;
  if (!aligned16(dz) || !aligned16(dw) || !aligned16(ws) || (db && !aligned16(db))) return RAI_E_UNSUPPORTED;
  if (first ? (!u8 && (reinterpret_cast<uintptr_t>(x) & 3)) : !aligned16(x)) return RAI_E_UNSUPPORTED;
  const int64_t M = B * H * W;
  const int pairs = wrw_pairs(Ci, Co);
  const int S = wrw_splits(M, pairs);
  const int64_t nw = (int64_t)Co * 9 * Ci;
  if (ws_bytes < (int64_t)S * (nw + Co) * 4) return RAI_E_WORKSPACE;
  C3WrwArgs a;
  a.x = x;
  a.xdiv = xdiv;
  a.dz = dz;
  a.part = reinterpret_cast<float*>(ws);
  a.M = M;
  a.chunk = ((M + S - 1) / S + 3) / 4 * 4;
  a.H = H;
  a.W = W;
  a.Ci = Ci;
  a.Co = Co;
  a.S = S;
  a.pre = pre;
  const dim3 grid((unsigned)(S / 4), (unsigned)pairs);
  if (!first) hipLaunchKernelGGL(conv3x3_wrw_kernel, grid, dim3(C3_THREADS), 0, st, a);
  else if (u8) hipLaunchKernelGGL(conv3x3_wrw_first_kernel<true>, grid, dim3(C3_THREADS), 0, st, a);
  else hipLaunchKernelGGL(conv3x3_wrw_first_kernel<false>, grid, dim3(C3_THREADS), 0, st, a);
  RAI_LAUNCH_CHECK();
  const int64_t n = nw + Co;
  hipLaunchKernelGGL(conv3x3_wrw_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a.part, S, nw,
                     Co, dw, db, accumulate);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

}  // namespace

extern "C" int rai_conv3x3_fwd(const float* x, const float* w, const float* b, const float* res, int64_t B, int32_t H,
                               int32_t W, int32_t Ci, int32_t Co, int32_t pre_relu, int32_t post_relu,
                               int32_t out_nchw, float* y, void* stream) {
  if (!x || !w || !b || !y) return RAI_E_NULLPTR;
  if (B < 0 || H < 1 || W < 1) return RAI_E_SHAPE;
  if (!chan_ok(Ci) || !chan_ok(Co)) return RAI_E_UNSUPPORTED;
  if (!aligned16(x) || !aligned16(w) || !aligned16(b) || !aligned16(y) || (res && !aligned16(res)))
    return RAI_E_UNSUPPORTED;
  C3Args a;
  a.x = x;
  a.w = w;
  a.b = b;
  a.m = nullptr;
  a.res = res;
  a.y = y;
  a.M = B * H * W;
  a.H = H;
  a.W = W;
  a.CK = Ci;
  a.CN = Co;
  a.pre = pre_relu != 0;
  a.post = post_relu != 0;
  a.nchw = out_nchw != 0;
  return launch_conv(a, false, rai_stream(stream));
}

extern "C" int rai_conv3x3_dgrad(const float* dz, const float* w, const float* m, const float* res, int64_t B,
                                 int32_t H, int32_t W, int32_t Ci, int32_t Co, float* dx, void* stream) {
  if (!dz || !w || !dx) return RAI_E_NULLPTR;
  if (B < 0 || H < 1 || W < 1) return RAI_E_SHAPE;
  if (!chan_ok(Ci) || !chan_ok(Co)) return RAI_E_UNSUPPORTED;
  if (!aligned16(dz) || !aligned16(w) || !aligned16(dx) || (m && !aligned16(m)) || (res && !aligned16(res)))
    return RAI_E_UNSUPPORTED;
  C3Args a;
  a.x = dz;
  a.w = w;
  a.b = nullptr;
  a.m = m;
  a.res = res;
  a.y = dx;
  a.M = B * H * W;
  a.H = H;
  a.W = W;
  a.CK = Co;
  a.CN = Ci;
  a.pre = 0;
  a.post = 0;
  a.nchw = 0;
  return launch_conv(a, true, rai_stream(stream));
}

extern "C" int rai_conv3x3_fwd_first(const void* x, int32_t x_is_u8, float x_divisor, const float* w, const float* b,
                                     int64_t B, int32_t H, int32_t W, int32_t Ci, int32_t Co, float* y,
                                     void* stream) {
  if (!x || !w || !b || !y) return RAI_E_NULLPTR;
  if (B < 0 || H < 1 || W < 1) return RAI_E_SHAPE;
  if ((Ci != 3 && Ci != 4) || !chan_ok(Co)) return RAI_E_UNSUPPORTED;
  if (x_is_u8 && !(x_divisor > 0.f)) return RAI_E_SHAPE;
  if (!aligned16(w) || !aligned16(b) || !aligned16(y) || (!x_is_u8 && (reinterpret_cast<uintptr_t>(x) & 3)))
    return RAI_E_UNSUPPORTED;
  C3FirstArgs a;
  a.x = x;
  a.xdiv = x_divisor;
  a.w = w;
  a.b = b;
  a.y = y;
  a.M = B * H * W;
  a.H = H;
  a.W = W;
  a.Ci = Ci;
  a.Co = Co;
  if (a.M == 0) return RAI_OK;
  const int64_t gx = (a.M + 255) / 256;
  if (gx > 0x7fffffffLL) return RAI_E_SHAPE;
  const dim3 grid((unsigned)gx, (unsigned)(Co / 16));
  hipStream_t st = rai_stream(stream);
  if (x_is_u8) hipLaunchKernelGGL(conv3x3_first_kernel<true>, grid, dim3(C3_THREADS), 0, st, a);
  else hipLaunchKernelGGL(conv3x3_first_kernel<false>, grid, dim3(C3_THREADS), 0, st, a);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_maxpool3x3s2_fwd(const float* x, int64_t B, int32_t H, int32_t W, int32_t C, float* y,
                                    uint8_t* argmax, void* stream) {
  if (!x || !y || !argmax) return RAI_E_NULLPTR;
  if (B < 0 || H < 1 || W < 1 || C < 1) return RAI_E_SHAPE;
  if (C % 4 || !aligned16(x) || !aligned16(y) || (reinterpret_cast<uintptr_t>(argmax) & 3)) return RAI_E_UNSUPPORTED;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const int64_t n4 = B * OH * OW * (C / 4);
  if (n4 == 0) return RAI_OK;
  const int64_t gx = (n4 + 255) / 256;
  if (gx > 0x7fffffffLL) return RAI_E_SHAPE;
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3((unsigned)gx), dim3(256), 0, rai_stream(stream), x, n4, H, W, C, OH, OW,
                     y, argmax);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_maxpool3x3s2_bwd(const float* dy, const uint8_t* argmax, int64_t B, int32_t H, int32_t W,
                                    int32_t C, float* dx, void* stream) {
  if (!dy || !dx || !argmax) return RAI_E_NULLPTR;
  if (B < 0 || H < 1 || W < 1 || C < 1) return RAI_E_SHAPE;
  if (C % 4 || !aligned16(dy) || !aligned16(dx) || (reinterpret_cast<uintptr_t>(argmax) & 3))
    return RAI_E_UNSUPPORTED;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const int64_t n4 = B * H * W * (C / 4);
  if (n4 == 0) return RAI_OK;
  const int64_t gx = (n4 + 255) / 256;
  if (gx > 0x7fffffffLL) return RAI_E_SHAPE;
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3((unsigned)gx), dim3(256), 0, rai_stream(stream), dy, argmax, n4, H, W, C,
                     OH, OW, dx);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int64_t rai_conv3x3_wgrad_workspace_bytes(int64_t B, int32_t H, int32_t W, int32_t Ci, int32_t Co) {
  if (B < 0 || H < 1 || W < 1 || !chan_ok(Co) || !(Ci == 3 || Ci == 4 || chan_ok(Ci))) return 0;
  const int S = wrw_splits(B * H * W, wrw_pairs(Ci, Co));
  return (int64_t)S * ((int64_t)Co * 9 * Ci + Co) * 4;
}

extern "C" int rai_conv3x3_wgrad(const float* x, const float* dz, int64_t B, int32_t H, int32_t W, int32_t Ci,
                                 int32_t Co, int32_t pre_relu, float* dw, float* db, int32_t accumulate,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  return wrw_common(x, false, false, 1.f, dz, B, H, W, Ci, Co, pre_relu != 0, dw, db, accumulate, workspace,
                    workspace_bytes, rai_stream(stream));
}

extern "C" int rai_conv3x3_wgrad_first(const void* x, int32_t x_is_u8, float x_divisor, const float* dz, int64_t B,
                                       int32_t H, int32_t W, int32_t Ci, int32_t Co, float* dw, float* db,
                                       int32_t accumulate, void* workspace, int64_t workspace_bytes, void* stream) {
  if (x_is_u8 && !(x_divisor > 0.f)) return RAI_E_SHAPE;
  return wrw_common(x, true, x_is_u8 != 0, x_divisor, dz, B, H, W, Ci, Co, 0, dw, db, accumulate, workspace,
                    workspace_bytes, rai_stream(stream));
}
