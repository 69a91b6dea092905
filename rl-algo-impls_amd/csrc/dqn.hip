// DQN on gfx950: device replay ring (push, keyed sample + gather), TD loss, fused output head, greedy
// argmax and the target-network update.  See include/rai_amd.h for the contract of each entry point.
//
// All of these are latency or bandwidth kernels (a DQN batch is 32..64 rows); none uses MFMA.  Built with
// -ffp-contract=off (build.py NO_CONTRACT): the TD target and the Polyak update follow torch's separately
// rounded multiply / add sequence bit for bit.
//
// In-launch inter-workgroup traffic is limited to one pattern: every workgroup reads the ring state at its
// start, and the LAST workgroup to arrive on an agent-scope counter writes the new state for the NEXT launch
// (which sees it across the kernel boundary).  No workgroup reads another's data within a launch; the one
// reduction across workgroups (the fused head's mean loss) is a second launch.
#include "common.h"

namespace {

constexpr int NT = 256;

// ---- copy granularity ---------------------------------------------------------------------------------
__host__ int copy_gran(int64_t row_bytes, uintptr_t align_bits) {
  if (row_bytes % 16 == 0 && align_bits % 16 == 0) return 16;
  if (row_bytes % 4 == 0 && align_bits % 4 == 0) return 4;
  return 1;
}
__device__ __forceinline__ void copy_unit(uint8_t* dst, const uint8_t* src, int64_t du, int64_t su, int gran) {
  if (gran == 16) reinterpret_cast<uint4*>(dst)[du] = reinterpret_cast<const uint4*>(src)[su];
  else if (gran == 4) reinterpret_cast<uint32_t*>(dst)[du] = reinterpret_cast<const uint32_t*>(src)[su];
  else dst[du] = src[su];
}

// The last workgroup to arrive returns true (thread 0 only) after re-arming the counter.  Every wave of the
// caller has consumed the state words it read (they are in its loop bounds and addresses) before the barrier.
__device__ __forceinline__ bool last_arrival(int32_t* counter) {
  __syncthreads();
  if (threadIdx.x != 0) return false;
  const int nb = (int)(gridDim.x * gridDim.y);
  if (__hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != nb - 1) return false;
  __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// ---- replay ring ---------------------------------------------------------------------------------------
struct RingDev {
  uint8_t* obs;
  uint8_t* next_obs;
  int64_t* actions;
  float* rewards;
  uint8_t* dones;
  int64_t capacity;
  int64_t units;  // granules per row
  int32_t gran;
  rai_replay_state* st;
};

struct PushArgs {
  RingDev r;
  const uint8_t* obs;
  const uint8_t* next_obs;
  const int64_t* actions;
  const float* rewards;
  const uint8_t* dones;
  int64_t N;
};

__global__ __launch_bounds__(NT) void replay_push_kernel(const PushArgs a) {
  rai_replay_state* st = a.r.st;
  const int64_t head = st->head, len = st->len, cap = a.r.capacity;
  const int64_t units = a.r.units, total = a.N * units;
  const int64_t stride = (int64_t)gridDim.x * NT;
  const int64_t t0 = (int64_t)blockIdx.x * NT + threadIdx.x;
  for (int64_t u = t0; u < total; u += stride) {
    const int64_t i = u / units, j = u - i * units;
    int64_t slot = head + i;
    if (slot >= cap) slot -= cap;  // head < cap and i < N <= cap
    copy_unit(a.r.obs, a.obs, slot * units + j, u, a.r.gran);
    copy_unit(a.r.next_obs, a.next_obs, slot * units + j, u, a.r.gran);
  }
  for (int64_t i = t0; i < a.N; i += stride) {
    int64_t slot = head + i;
    if (slot >= cap) slot -= cap;
    a.r.actions[slot] = a.actions[i];
    a.r.rewards[slot] = a.rewards[i];
    a.r.dones[slot] = a.dones[i];
  }
  if (last_arrival(&st->arrivals)) {
    int64_t nh = head + a.N;
    if (nh >= cap) nh -= cap;
    const int64_t nl = len + a.N < cap ? len + a.N : cap;
    __hip_atomic_store(&st->head, nh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&st->len, nl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The keyed bijection of rai_feistel_permutation (rollout.hip): the same mix, rounds, key schedule and
// domain split, evaluated for ONE index with n read on the device (tests compare the two for B == len).
__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
constexpr int ROUNDS = 6;
__device__ __forceinline__ int64_t feistel_index(int64_t i, int64_t n, uint64_t key) {
  int bits = n > 1 ? 64 - __clzll((unsigned long long)(n - 1)) : 0;
  if (bits < 2) bits = 2;
  const int h1 = bits / 2, h2 = bits - h1;
  const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
  uint32_t k[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) k[r] = mix32(klo ^ mix32(khi + 0x9e3779b9u * (uint32_t)(r + 1)));
  const uint32_t m1 = (1u << h1) - 1u, m2 = (1u << h2) - 1u;
  uint64_t x = (uint64_t)i;
  do {  // the domain 2^bits is < 2n (n >= 3) or 4 (n <= 2): a short walk back into [0, n)
    uint32_t hi = (uint32_t)(x >> h2), lo = (uint32_t)x & m2;
#pragma unroll
    for (int r = 0; r < ROUNDS; r += 2) {
      const uint32_t t = hi ^ (mix32(lo ^ k[r]) & m1);
      hi = lo;
      lo = t;
      const uint32_t u = hi ^ (mix32(lo ^ k[r + 1]) & m2);
      hi = lo;
      lo = u;
    }
    x = ((uint64_t)hi << h2) | lo;
  } while (x >= (uint64_t)n);
  return (int64_t)x;
}

struct SampleArgs {
  RingDev r;
  uint64_t seed;
  const int64_t* inject;
  int64_t* slots;
  uint8_t* obs;
  uint8_t* next_obs;
  int64_t* actions;
  float* rewards;
  uint8_t* dones;
  int64_t B;
  int32_t gather;
};

// grid (splits, B): workgroup (s, b) copies share s of batch row b.
__global__ __launch_bounds__(NT) void replay_sample_kernel(const SampleArgs a) {
  rai_replay_state* st = a.r.st;
  const int64_t head = st->head, len = st->len, draws = st->draws, cap = a.r.capacity;
  const int64_t b = blockIdx.y;
  if (a.B > len) {  // every workgroup takes this exit: nothing arrives on the counter
    if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) st->err = 1;
    return;
  }
  int64_t pos;
  bool ok = true;
  if (a.inject) {
    pos = a.inject[b];
    ok = pos >= 0 && pos < len;
    if (!ok && blockIdx.x == 0 && threadIdx.x == 0) st->err = 2;
  } else {
    pos = feistel_index(b, len, a.seed + 0x9E3779B97F4A7C15ull * (uint64_t)draws);
  }
  if (ok) {
    int64_t slot = head - len + pos;  // in (-cap, cap)
    if (slot < 0) slot += cap;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (a.slots) a.slots[b] = slot;
      if (a.gather) {
        a.actions[b] = a.r.actions[slot];
        a.rewards[b] = a.r.rewards[slot];
        a.dones[b] = a.r.dones[slot];
      }
    }
    if (a.gather) {
      const int64_t units = a.r.units;
      for (int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x; j < units; j += (int64_t)gridDim.x * NT) {
        copy_unit(a.obs, a.r.obs, b * units + j, slot * units + j, a.r.gran);
        copy_unit(a.next_obs, a.r.next_obs, b * units + j, slot * units + j, a.r.gran);
      }
    }
  }
  if (!a.inject && last_arrival(&st->arrivals))
    __hip_atomic_store(&st->draws, draws + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int ring_dev(const rai_replay_ring* ring, uintptr_t extra_align, RingDev* out) {
  if (!ring) return RAI_E_NULLPTR;
  if (ring->capacity < 1 || ring->row_bytes < 1) return RAI_E_SHAPE;
  if (!ring->obs || !ring->next_obs || !ring->actions || !ring->rewards || !ring->dones || !ring->state)
    return RAI_E_NULLPTR;
  const uintptr_t al = (uintptr_t)ring->obs | (uintptr_t)ring->next_obs | extra_align;
  out->obs = static_cast<uint8_t*>(ring->obs);
  out->next_obs = static_cast<uint8_t*>(ring->next_obs);
  out->actions = ring->actions;
  out->rewards = ring->rewards;
  out->dones = ring->dones;
  out->capacity = ring->capacity;
  out->gran = copy_gran(ring->row_bytes, al);
  out->units = ring->row_bytes / out->gran;
  out->st = ring->state;
  return RAI_OK;
}

// ---- TD loss -------------------------------------------------------------------------------------------
// torch.max over a row: the larger value, NaN wins.
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ float wave_nan_max(float m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  return m;
}

struct TdRow {
  float target, loss, g;
};
// dqn.py:115-117 for one row; inv_b = 1.0f / (float)B: the mean's gradient is a multiply by the rounded
// reciprocal, as torch's smooth_l1 backward (norm = 1 / numel) and its device division by a scalar are.
__device__ __forceinline__ TdRow td_row(float qsel, float qmax, float r, uint8_t done, float gamma, float inv_b) {
  const float nd = done ? 0.0f : 1.0f;     // ~d as a float
  const float t = r + ((nd * gamma) * qmax);  // separately rounded (-ffp-contract=off)
  const float d = qsel - t;
  const float ad = fabsf(d);
  TdRow o;
  o.target = t;
  o.loss = ad < 1.0f ? 0.5f * d * d : ad - 0.5f;    // smooth_l1, beta = 1 (NaN falls through as NaN)
  o.g = (d < -1.0f ? -1.0f : (d > 1.0f ? 1.0f : d)) * inv_b;  // clamp keeps NaN, as torch.clamp
  return o;
}

constexpr int TD_NT = 1024;
__global__ __launch_bounds__(TD_NT) void td_loss_kernel(const float* __restrict__ q, const float* __restrict__ qn,
                                                        const int64_t* __restrict__ actions,
                                                        const float* __restrict__ rewards,
                                                        const uint8_t* __restrict__ dones, int64_t B, int A,
                                                        float gamma, float* __restrict__ target,
                                                        float* __restrict__ loss, float* __restrict__ dq) {
  __shared__ double part[TD_NT / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = TD_NT / 64;
  const float inv_b = 1.0f / (float)B;
  double acc = 0.0;  // this wave's rows b = w, w + nw, ... in ascending order
  for (int64_t b = w; b < B; b += nw) {
    float m = -INFINITY;
    for (int a = lane; a < A; a += 64) m = nan_max(m, qn[b * A + a]);
    m = wave_nan_max(m);
    const int64_t ab = actions[b];
    const bool in = ab >= 0 && ab < A;
    const float qsel = in ? q[b * A + ab] : NAN;
    const TdRow o = td_row(qsel, m, rewards[b], dones[b], gamma, inv_b);
    for (int a = lane; a < A; a += 64) dq[b * A + a] = a == ab ? o.g : 0.0f;
    if (lane == 0) target[b] = o.target;
    acc += (double)o.loss;
  }
  if (lane == 0) part[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < nw; ++i) s += part[i];
    loss[0] = (float)(s / (double)B);
  }
}

// ---- fused output head ---------------------------------------------------------------------------------
// One workgroup per batch row: both rows of activations in LDS; wave w takes dot products w, w + 4, ...
// (tasks [0, A): the target network's outputs; [A, 2A): the online network's, of which only a_b is needed
// unless q_out is requested).  A dot product is lane-strided over H (coalesced weight rows) and summed by
// the fixed-order wave reduction.
__global__ __launch_bounds__(NT) void dqn_head_fwd_kernel(
    const float* __restrict__ h, const float* __restrict__ hn, const float* __restrict__ w,
    const float* __restrict__ bias, const float* __restrict__ wt, const float* __restrict__ bt,
    const int64_t* __restrict__ actions, const float* __restrict__ rewards, const uint8_t* __restrict__ dones,
    int64_t B, int H, int A, float gamma, float* __restrict__ target, float* __restrict__ g,
    float* __restrict__ q_out, float* __restrict__ qn_out, float* __restrict__ row_loss) {
  __shared__ float hs[2][RAI_DQN_HEAD_MAX_H];
  __shared__ float qs[2][RAI_DQN_HEAD_MAX_A];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < H; k += NT) {
    hs[0][k] = hn[b * H + k];
    hs[1][k] = h[b * H + k];
  }
  const int64_t ab = actions[b];
  const bool in = ab >= 0 && ab < A;
  __syncthreads();
  for (int t = wv; t < 2 * A; t += NT / 64) {
    const int net = t >= A, a = net ? t - A : t;
    if (net && !q_out && a != ab) continue;  // wave-uniform
    const float* row = (net ? w : wt) + (int64_t)a * H;
    float s = 0.0f;
    for (int k = lane; k < H; k += 64) s += hs[net][k] * row[k];
    s = wave_sum(s);
    if (lane == 0) qs[net][a] = s + (net ? bias[a] : bt[a]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float m = -INFINITY;
    for (int a = 0; a < A; ++a) m = nan_max(m, qs[0][a]);
    const TdRow o = td_row(in ? qs[1][ab] : NAN, m, rewards[b], dones[b], gamma, 1.0f / (float)B);
    target[b] = o.target;
    g[b] = o.g;
    row_loss[b] = o.loss;
  }
  if (threadIdx.x < A) {
    if (qn_out) qn_out[b * A + threadIdx.x] = qs[0][threadIdx.x];
    if (q_out) q_out[b * A + threadIdx.x] = qs[1][threadIdx.x];
  }
}

// mean of row_loss in a fixed order: lane-strided ascending partials in double, then the wave tree.
__global__ __launch_bounds__(64) void mean_rows_kernel(const float* __restrict__ x, int64_t B, float* __restrict__ out) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < B; i += 64) s += (double)x[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) out[0] = (float)(s / (double)B);
}

// Workgroups [0, B): dh row b.  Workgroups [B, B + A): action a's weight row and bias gradient, each thread
// one column j, summing the matching rows in ascending b.
__global__ __launch_bounds__(NT) void dqn_head_bwd_kernel(const float* __restrict__ h, const float* __restrict__ w,
                                                          const int64_t* __restrict__ actions,
                                                          const float* __restrict__ g, int64_t B, int H, int A,
                                                          float* __restrict__ dh, float* __restrict__ dw,
                                                          float* __restrict__ db, int accumulate) {
  const int64_t blk = blockIdx.x;
  if (blk < B) {
    const int64_t ab = actions[blk];
    const float gb = g[blk];
    const bool in = ab >= 0 && ab < A;
    for (int j = threadIdx.x; j < H; j += NT) dh[blk * H + j] = in ? gb * w[ab * H + j] : NAN;
    return;
  }
  const int64_t a = blk - B;
  for (int j = threadIdx.x; j < H; j += NT) {
    float acc = 0.0f;
    for (int64_t b = 0; b < B; ++b)
      if (actions[b] == a) acc += g[b] * h[b * H + j];
    dw[a * H + j] = accumulate ? dw[a * H + j] + acc : acc;
  }
  if (threadIdx.x == 0) {
    float acc = 0.0f;
    for (int64_t b = 0; b < B; ++b)
      if (actions[b] == a) acc += g[b];
    db[a] = accumulate ? db[a] + acc : acc;
  }
}

// ---- argmax ----------------------------------------------------------------------------------------------
// (value, index) order of torch.argmax: NaN above everything, then the larger value, then the lower index.
__device__ __forceinline__ bool arg_better(float v, int i, float bv, int bi) {
  if (bi < 0) return i >= 0;
  if (i < 0) return false;
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (!vn && v != bv) return v > bv;
  return i < bi;
}
__global__ __launch_bounds__(NT) void argmax_rows_kernel(const float* __restrict__ x, int64_t B, int A,
                                                         int64_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  if (b >= B) return;  // whole waves
  float bv = 0.0f;
  int bi = -1;
  for (int a = lane; a < A; a += 64) {
    const float v = x[b * A + a];
    if (arg_better(v, a, bv, bi)) {
      bv = v;
      bi = a;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (arg_better(ov, oi, bv, bi)) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) out[b] = bi;
}

// ---- Polyak ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float polyak1(float t, float p, float tau, float omt) { return (tau * p) + (omt * t); }
__global__ __launch_bounds__(NT) void polyak_kernel(float* __restrict__ target, const float* __restrict__ p,
                                                    int64_t n, float tau, float omt, int copy, int vec) {
  const int64_t stride = (int64_t)gridDim.x * NT, t0 = (int64_t)blockIdx.x * NT + threadIdx.x;
  const int64_t n4 = vec ? n / 4 : 0;
  for (int64_t i = t0; i < n4; i += stride) {
    const float4 pv = reinterpret_cast<const float4*>(p)[i];
    float4 tv = pv;
    if (!copy) {
      tv = reinterpret_cast<float4*>(target)[i];
      tv.x = polyak1(tv.x, pv.x, tau, omt);
      tv.y = polyak1(tv.y, pv.y, tau, omt);
      tv.z = polyak1(tv.z, pv.z, tau, omt);
      tv.w = polyak1(tv.w, pv.w, tau, omt);
    }
    reinterpret_cast<float4*>(target)[i] = tv;
  }
  for (int64_t i = 4 * n4 + t0; i < n; i += stride) target[i] = copy ? p[i] : polyak1(target[i], p[i], tau, omt);
}

}  // namespace

extern "C" int rai_replay_push(const rai_replay_ring* ring, const void* obs, const void* next_obs,
                               const int64_t* actions, const float* rewards, const uint8_t* dones, int64_t N,
                               void* stream) {
  PushArgs a;
  const int rc = ring_dev(ring, (uintptr_t)obs | (uintptr_t)next_obs, &a.r);
  if (rc != RAI_OK) return rc;
  if (N < 0 || N > ring->capacity) return RAI_E_SHAPE;
  if (N == 0) return RAI_OK;
  if (!obs || !next_obs || !actions || !rewards || !dones) return RAI_E_NULLPTR;
  a.obs = static_cast<const uint8_t*>(obs);
  a.next_obs = static_cast<const uint8_t*>(next_obs);
  a.actions = actions;
  a.rewards = rewards;
  a.dones = dones;
  a.N = N;
  int64_t blocks = (N * a.r.units + NT - 1) / NT;
  if (blocks > 64) blocks = 64;  // every workgroup arrives on one counter
  hipLaunchKernelGGL(replay_push_kernel, dim3((unsigned)blocks), dim3(NT), 0, rai_stream(stream), a);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_replay_sample(const rai_replay_ring* ring, uint64_t seed, int64_t B, const int64_t* inject,
                                 int64_t* slots_out, void* obs_out, void* next_obs_out, int64_t* actions_out,
                                 float* rewards_out, uint8_t* dones_out, void* stream) {
  SampleArgs a;
  const int rc = ring_dev(ring, (uintptr_t)obs_out | (uintptr_t)next_obs_out, &a.r);
  if (rc != RAI_OK) return rc;
  if (B < 1 || B > ring->capacity || B > 65535) return RAI_E_SHAPE;
  const int n_out = (obs_out != nullptr) + (next_obs_out != nullptr) + (actions_out != nullptr) +
                    (rewards_out != nullptr) + (dones_out != nullptr);
  if (n_out != 0 && n_out != 5) return RAI_E_NULLPTR;
  if (n_out == 0 && !slots_out) return RAI_E_NULLPTR;
  a.seed = seed;
  a.inject = inject;
  a.slots = slots_out;
  a.obs = static_cast<uint8_t*>(obs_out);
  a.next_obs = static_cast<uint8_t*>(next_obs_out);
  a.actions = actions_out;
  a.rewards = rewards_out;
  a.dones = dones_out;
  a.B = B;
  a.gather = n_out == 5;
  // a row's granules over up to 8 workgroups (a 28 KB Atari frame: 1,764 16-byte granules)
  int64_t splits = a.gather ? (a.r.units + 4 * NT - 1) / (4 * NT) : 1;
  if (splits > 8) splits = 8;
  if (splits < 1) splits = 1;
  hipLaunchKernelGGL(replay_sample_kernel, dim3((unsigned)splits, (unsigned)B), dim3(NT), 0, rai_stream(stream), a);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_dqn_td_loss(const float* q, const float* q_next_target, const int64_t* actions,
                               const float* rewards, const uint8_t* dones, int64_t B, int32_t A, float gamma,
                               float* target_out, float* loss_out, float* dq_out, void* stream) {
  if (B < 1 || A < 1) return RAI_E_SHAPE;
  if (A > RAI_DQN_MAX_A) return RAI_E_UNSUPPORTED;
  if (!q || !q_next_target || !actions || !rewards || !dones || !target_out || !loss_out || !dq_out)
    return RAI_E_NULLPTR;
  hipLaunchKernelGGL(td_loss_kernel, dim3(1), dim3(TD_NT), 0, rai_stream(stream), q, q_next_target, actions,
                     rewards, dones, B, (int)A, gamma, target_out, loss_out, dq_out);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int64_t rai_dqn_head_workspace_bytes(int64_t B) { return B < 1 ? 0 : 4 * B; }

extern "C" int rai_dqn_head_fwd(const float* h, const float* h_next, const float* w, const float* b,
                                const float* wt, const float* bt, const int64_t* actions, const float* rewards,
                                const uint8_t* dones, int64_t B, int32_t H, int32_t A, float gamma,
                                float* target_out, float* loss_out, float* g_out, float* q_out, float* q_next_out,
                                void* workspace, int64_t workspace_bytes, void* stream) {
  if (B < 1 || H < 1 || A < 1 || B > 0x7fffffff) return RAI_E_SHAPE;
  if (H > RAI_DQN_HEAD_MAX_H || A > RAI_DQN_HEAD_MAX_A) return RAI_E_UNSUPPORTED;
  if (!h || !h_next || !w || !b || !wt || !bt || !actions || !rewards || !dones || !target_out || !loss_out ||
      !g_out || !workspace)
    return RAI_E_NULLPTR;
  if (workspace_bytes < rai_dqn_head_workspace_bytes(B)) return RAI_E_WORKSPACE;
  float* row_loss = static_cast<float*>(workspace);
  hipLaunchKernelGGL(dqn_head_fwd_kernel, dim3((unsigned)B), dim3(NT), 0, rai_stream(stream), h, h_next, w, b, wt,
                     bt, actions, rewards, dones, B, (int)H, (int)A, gamma, target_out, g_out, q_out, q_next_out,
                     row_loss);
  RAI_LAUNCH_CHECK();
  hipLaunchKernelGGL(mean_rows_kernel, dim3(1), dim3(64), 0, rai_stream(stream), row_loss, B, loss_out);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_dqn_head_bwd(const float* h, const float* w, const int64_t* actions, const float* g, int64_t B,
                                int32_t H, int32_t A, float* dh, float* dw, float* db, int32_t accumulate,
                                void* stream) {
  if (B < 1 || H < 1 || A < 1 || B > 0x7fffff00) return RAI_E_SHAPE;
  if (H > RAI_DQN_HEAD_MAX_H || A > RAI_DQN_HEAD_MAX_A) return RAI_E_UNSUPPORTED;
  if (!h || !w || !actions || !g || !dh || !dw || !db) return RAI_E_NULLPTR;
  hipLaunchKernelGGL(dqn_head_bwd_kernel, dim3((unsigned)(B + A)), dim3(NT), 0, rai_stream(stream), h, w, actions, g,
                     B, (int)H, (int)A, dh, dw, db, (int)accumulate);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_argmax_rows(const float* x, int64_t B, int32_t A, int64_t* out, void* stream) {
  if (B < 0 || A < 1 || B > 0x7fffff00) return RAI_E_SHAPE;
  if (B == 0) return RAI_OK;
  if (!x || !out) return RAI_E_NULLPTR;
  const int64_t blocks = (B + NT / 64 - 1) / (NT / 64);
  hipLaunchKernelGGL(argmax_rows_kernel, dim3((unsigned)blocks), dim3(NT), 0, rai_stream(stream), x, B, (int)A, out);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

extern "C" int rai_polyak_update(float* target, const float* params, int64_t n, double tau, double one_minus_tau,
                                 void* stream) {
  if (n < 0) return RAI_E_SHAPE;
  if (n == 0) return RAI_OK;
  if (!target || !params) return RAI_E_NULLPTR;
  const int vec = (((uintptr_t)target | (uintptr_t)params) % 16) == 0;
  int64_t blocks = ((vec ? n / 4 : n) + NT - 1) / NT;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(polyak_kernel, dim3((unsigned)blocks), dim3(NT), 0, rai_stream(stream), target, params, n,
                     (float)tau, (float)one_minus_tau, tau == 1.0 ? 1 : 0, vec);
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}
