// Ingest of a scripted bot's recorded actions (the reference-AI rollout generator) on gfx950.
//
// rl_algo_impls/rollout/reference_ai_rollout.py:69-70 folds vec_env.last_action into the rollout's action
// buffer as the env handed it over.  The update kernels index a row's logits by these values, so here the
// hand-over is one launch per env step that widens (int32 or int64 source -> the buffers' int64), sanitises
// and counts:
//   out of range (a < 0 or a >= nvec[g], compared at the source's full width): 0 is stored, counted;
//   masked out (in range, the group's mask slice has a true entry, the action's entry is false): stored
//   unchanged, counted;
//   anything else: stored unchanged.
// bad[n] is env n's count.
//
// Layout: src / dst are (R, G) row-major, R = N * cells rows; mask (R, A) bytes, A = sum(nvec).  Rows are
// walked in tiles of 64, whose mask bytes are one contiguous span (at most 16 KiB, A <= 256) staged into LDS
// by 16-byte loads from the span's first 16-byte-aligned address on (single bytes before and after it; the
// LDS copy starts at the same offset within 16 bytes as the span does in memory, so the vector stores are
// aligned too).  cells > 1: one 256-thread workgroup per env, the tile's (row, group) components spread over
// the threads (consecutive threads read and write consecutive components), the env's count a fixed-order
// block sum.  cells == 1: a workgroup takes 256 envs and a thread one whole row, so an env's count never
// leaves a register; the 256 rows are staged in one pass when they fit the tile (A <= 64), else as four
// tiles of 64 rows with wave w owning tile w.  Either way bad[n] is written once by an
// ordinary store: no atomics, nothing to zero beforehand, two calls give the same bits.
#include "common.h"

namespace {

constexpr int RA_THREADS = 256;
constexpr int RA_ROWS = 64;  // rows per LDS tile
constexpr int RA_MAX_G = RAI_MD_MAX_G, RA_MAX_A = RAI_GRID_MAX_A;
constexpr int RA_TILE_VEC = RA_ROWS * RA_MAX_A / 16 + 1;  // uint4 words: the largest span and its 15-byte shift
constexpr int RA_BATCH = 4;                                // 16-byte loads in flight per thread

struct RefActArgs {
  const void* src;
  const uint8_t* mask;  // null: nothing is masked out
  int64_t* dst;
  int32_t* bad;
  int64_t N;
  int32_t cells, G, A;
  uint16_t off[RA_MAX_G + 1];  // group g: mask entries [off[g], off[g + 1])
};

// `span` mask bytes from p into LDS at tile + (p & 15).  Every load lies inside [p, p + span).
__device__ __forceinline__ const uint8_t* load_mask_tile(const uint8_t* __restrict__ p, int span, uint4* tile,
                                                         int tid) {
  const int shift = (int)(reinterpret_cast<uintptr_t>(p) & 15);
  uint8_t* t = reinterpret_cast<uint8_t*>(tile) + shift;
  const int head = min((16 - shift) & 15, span);
  const int nvec16 = (span - head) >> 4;
  const int tail0 = head + (nvec16 << 4);
  if (tid < head) t[tid] = p[tid];
  if (tid >= RA_THREADS - 16 && tail0 + (tid - (RA_THREADS - 16)) < span) {
    const int i = tail0 + (tid - (RA_THREADS - 16));
    t[i] = p[i];
  }
  const uint4* __restrict__ g4 = reinterpret_cast<const uint4*>(p + head);
  uint4* t4 = reinterpret_cast<uint4*>(t + head);
  for (int k0 = tid; k0 < nvec16; k0 += RA_BATCH * RA_THREADS) {
    uint4 v[RA_BATCH];
#pragma unroll
    for (int k = 0; k < RA_BATCH; ++k) v[k] = g4[min(k0 + k * RA_THREADS, nvec16 - 1)];
#pragma unroll
    for (int k = 0; k < RA_BATCH; ++k)
      if (k0 + k * RA_THREADS < nvec16) t4[k0 + k * RA_THREADS] = v[k];
  }
  return t;
}

// One component: the value to store and whether it counts.  m: the row's mask bytes (LDS) or null.
template <typename SrcT>
__device__ __forceinline__ int64_t sanitise(SrcT a, const uint8_t* m, int lo, int n, int& count) {
  if (a < (SrcT)0 || a >= (SrcT)n) {
    ++count;
    return 0;
  }
  if (m) {
    bool any = false;
    for (int j = 0; j < n; ++j) any = any || m[lo + j] != 0;
    if (any && m[lo + (int)a] == 0) ++count;
  }
  return (int64_t)a;
}

template <typename SrcT, bool SINGLE>
__global__ __launch_bounds__(RA_THREADS) void ref_actions_kernel(const RefActArgs a) {
  __shared__ uint4 tile[RA_TILE_VEC];
  __shared__ int red[RA_THREADS / 64];
  const SrcT* __restrict__ src = static_cast<const SrcT*>(a.src);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int G = a.G, A = a.A;
  if (SINGLE) {
    // rows are envs: this workgroup's are [row0, row0 + 256).  Their mask bytes fit the LDS tile in one pass
    // when A <= 64 (every Discrete space, most MultiDiscrete ones; also when there is no mask): every thread
    // then takes one row.  Wider rows go in four tiles of 64, tile i processed by wave i.
    const int64_t row0 = (int64_t)blockIdx.x * RA_THREADS;
    const int TR = (!a.mask || A * RA_THREADS <= RA_ROWS * RA_MAX_A) ? RA_THREADS : RA_ROWS;  // rows per tile
    for (int i = 0; i < RA_THREADS / TR; ++i) {
      const int64_t t0 = row0 + (int64_t)i * TR;
      if (t0 >= a.N) break;  // uniform over the workgroup
      const int nr = (int)min((int64_t)TR, a.N - t0);
      const uint8_t* mt = nullptr;
      if (a.mask) {
        mt = load_mask_tile(a.mask + t0 * A, nr * A, tile, tid);
        __syncthreads();
      }
      const int rl = TR == RA_THREADS ? tid : lane;  // this thread's row of the tile
      if ((TR == RA_THREADS || w == i) && rl < nr) {
        const int64_t r = t0 + rl;
        int count = 0;
        for (int g = 0; g < G; ++g) {
          const int lo = a.off[g], n = a.off[g + 1] - lo;
          a.dst[r * G + g] = sanitise<SrcT>(src[r * G + g], mt ? mt + rl * A : nullptr, lo, n, count);
        }
        a.bad[r] = count;
      }
      if (a.mask) __syncthreads();  // the tile is read before the next one is staged
    }
  } else {
    const int64_t env = blockIdx.x;
    const int C = a.cells;
    int count = 0;
    for (int c0 = 0; c0 < C; c0 += RA_ROWS) {
      const int nr = min(RA_ROWS, C - c0);
      const int64_t r0 = env * C + c0;
      const uint8_t* mt = nullptr;
      if (a.mask) {
        mt = load_mask_tile(a.mask + r0 * A, nr * A, tile, tid);
        __syncthreads();
      }
      const int items = nr * G;
      for (int it = tid; it < items; it += RA_THREADS) {
        const int rl = it / G, g = it - rl * G;
        const int lo = a.off[g], n = a.off[g + 1] - lo;
        const int64_t i = r0 * G + it;
        a.dst[i] = sanitise<SrcT>(src[i], mt ? mt + rl * A : nullptr, lo, n, count);
      }
      if (a.mask) __syncthreads();
    }
    // fixed-order block sum (integers: any order is exact)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
    if (lane == 0) red[w] = count;
    __syncthreads();
    if (tid == 0) {
      int s = 0;
      for (int i = 0; i < RA_THREADS / 64; ++i) s += red[i];
      a.bad[env] = s;
    }
  }
}

template <typename SrcT>
int launch(const RefActArgs& a, hipStream_t st) {
  if (a.cells == 1) {
    const int64_t blocks = (a.N + RA_THREADS - 1) / RA_THREADS;
    hipLaunchKernelGGL((ref_actions_kernel<SrcT, true>), dim3((unsigned)blocks), dim3(RA_THREADS), 0, st, a);
  } else {
    hipLaunchKernelGGL((ref_actions_kernel<SrcT, false>), dim3((unsigned)a.N), dim3(RA_THREADS), 0, st, a);
  }
  RAI_LAUNCH_CHECK();
  return RAI_OK;
}

}  // namespace

extern "C" int rai_ref_actions_store(const void* src, int32_t src_dtype, const int32_t* nvec, int32_t G,
                                     const uint8_t* mask, int64_t N, int32_t cells, int64_t* dst, int32_t* bad,
                                     void* stream) {
  if (N < 0 || cells < 1 || G < 1 || G > RA_MAX_G) return RAI_E_SHAPE;
  if (src_dtype != RAI_REF_ACT_I32 && src_dtype != RAI_REF_ACT_I64) return RAI_E_SHAPE;
  if (!nvec) return RAI_E_NULLPTR;
  RefActArgs a{};
  int64_t A = 0;
  for (int g = 0; g < G; ++g) {
    if (nvec[g] < 1) return RAI_E_SHAPE;
    A += nvec[g];
    if (A > RA_MAX_A) return RAI_E_UNSUPPORTED;
    a.off[g + 1] = (uint16_t)A;
  }
  if (N > 0x7fffffffLL) return RAI_E_SHAPE;  // the grid of the cells > 1 form
  if (N == 0) return RAI_OK;
  if (!src || !dst || !bad) return RAI_E_NULLPTR;
  a.src = src;
  a.mask = mask;
  a.dst = dst;
  a.bad = bad;
  a.N = N;
  a.cells = cells;
  a.G = G;
  a.A = (int32_t)A;
  return src_dtype == RAI_REF_ACT_I32 ? launch<int32_t>(a, rai_stream(stream))
                                      : launch<int64_t>(a, rai_stream(stream));
}
