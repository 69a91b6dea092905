// Shared by the fused PPO epoch kernels of mlp_ppo.hip (mlp_net.h: one CU per network; mlp_mc.h: 4;
// mlp_mc8.h: 8 or 16): the phase stamps and lane idiom, the small device helpers, clip_grad_norm_'s
// coefficient and the stat-row writer (all three kernels); the weight layout of LDS / partial-gradient
// buffers / exchange slots, the cross-GPU exchange region, and the phases the two multi-CU kernels run
// the same way (weights and Adam moments in, per-CU stat partials, stat rows, write-back).  Included
// once, inside mlp_ppo.hip's anonymous namespace, after ppo_row_loss.h and before the kernel headers
// (uses HID, LD, f4, MlpArgs, RowLossHp and common.h).

#ifdef RAI_STAMPS
// Diagnostic build only (never the shipped library): per-phase cycle totals of wave 0 of
// each workgroup, accumulated over the launch and copied out by rai_mlp_debug_stamps().
__device__ unsigned long long g_stamps[2][32];
#define STAMP(i)                                                                 \
  do {                                                                           \
    if (threadIdx.x == 0) {                                                      \
      unsigned long long t_;                                                     \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
      S.stamps[i] += t_ - S.t_last;                                              \
      S.t_last = t_;                                                             \
    }                                                                            \
  } while (0)
#else
#define STAMP(i) \
  do {           \
  } while (0)
#endif

// Re-derive the lane coordinates inside each phase from a freshly computed lane id (mbcnt, so
// threadIdx.x's register need not stay live) and an opaque copy of the wave index, so the
// compiler recomputes per-phase LDS addresses where they are used instead of hoisting them all
// out of the minibatch loop (which overflows 128 VGPRs and spills).
#define RELANE()                                                                     \
  int tid_l_ = (w << 6) | (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); \
  asm volatile("" : "+v"(tid_l_));                                                   \
  int w_l_ = w;                                                                      \
  asm volatile("" : "+s"(w_l_));                                                     \
  const int tid = tid_l_, lane = tid & 63, g = lane >> 4, li = lane & 15, w = w_l_;  \
  (void)tid; (void)lane; (void)g; (void)li; (void)w

__device__ __forceinline__ int kmap(int g, int kk) { return (g & 1) * 32 + (g >> 1) * 16 + kk; }
__device__ __forceinline__ int smap(int g, int kk) {
  return (kk >> 3) * 32 + (g >> 1) * 16 + (g & 1) * 8 + (kk & 7);
}
// Branch-free tanh (libm's tanhf branches on |x| ranges, which diverges across a wave):
// |x| < 0.3: odd Taylor series to x^9 (truncation < 1e-7 relative); otherwise
// 1 - 2 / (exp(2|x|) + 1) with the sign restored (absolute error ~1 ulp of 1).
__device__ __forceinline__ float tanh_bf(float x) {
  const float ax = fabsf(x);
  const float x2 = x * x;
  float p = fmaf(x2, 62.f / 2835.f, -17.f / 315.f);
  p = fmaf(x2, p, 2.f / 15.f);
  p = fmaf(x2, p, -1.f / 3.f);
  const float small = fmaf(x * x2, p, x);
  const float e = __builtin_amdgcn_exp2f(ax * 2.885390081777927f);  // exp(2|x|)
  const float big = fmaf(-2.f, __builtin_amdgcn_rcpf(e + 1.f), 1.f);
  return ax < 0.3f ? small : copysignf(big, x);
}
__device__ __forceinline__ float act_f(const int relu, float z) { return relu ? fmaxf(z, 0.f) : tanh_bf(z); }
__device__ __forceinline__ float act_d(int relu, float h) { return relu ? (h > 0.f ? 1.f : 0.f) : 1.f - h * h; }

// Sum over the 16 lanes of a DPP row; every lane of the row receives the same bits.
template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row_sum16(float v) {
  v += dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp<0x141>(v);  // row_half_mirror
  v += dpp<0x140>(v);  // row_mirror
  return v;
}

// clip_grad_norm_'s coefficient for the global gradient norm
__device__ __forceinline__ float clip_coef(float max_grad_norm, float total_norm) {
  float coef = 1.f;
  if (max_grad_norm > 0.f) coef = fminf(max_grad_norm / (total_norm + 1e-6f), 1.f);
  return coef;
}

// One network's columns of a minibatch's stat row from its four fp64 sums over the minibatch's rows
// (ppo_row_loss's st, summed over every rank's share of the rows by the host for world > 1)
template <bool ACTOR>
__device__ __forceinline__ void stat_row_write(float* row, const double (&sv)[4], int rows, int world,
                                               const RowLossHp& lh) {
  const double Bd = (double)rows * (double)world;
  if (ACTOR) {
    const float pi_loss = (float)(-sv[0] / Bd);
    const float ent_loss = (float)(-sv[3] / Bd);
    row[0] = lh.pi_coef * pi_loss + lh.ent_coef * ent_loss;  // host adds the value term
    row[1] = pi_loss;
    row[2] = ent_loss;
    row[3] = (float)(sv[1] / Bd);
    row[4] = (float)(sv[2] / Bd);
  } else {
    row[5] = (float)(sv[0] / Bd) * lh.halve;
    row[5 + RAI_MAX_K] = lh.has_vclip ? (float)(sv[1] / Bd) : 0.f;
  }
}

// ---- the multi-CU kernels (mlp_mc.h, mlp_mc8.h) ----------------------------------------------------

constexpr int MC_NT = 256;           // threads per CU (4 waves, one per SIMD)
constexpr int MC_NW = MC_NT / 64;

// Weight layout shared by LDS, the partial-gradient buffers and the exchange slots (floats).
constexpr int WL_W1 = 0;                   // [64][4]
constexpr int WL_B1 = WL_W1 + HID * 4;     // [64]
constexpr int WL_W2 = WL_B1 + HID;         // [64][LD]
constexpr int WL_B2 = WL_W2 + HID * LD;    // [64]
constexpr int WL_W3 = WL_B2 + HID;         // [OUTP][LD]
constexpr int WL_N = 4752;                 // >= WL_W3 + 2 * LD + 8, multiple of 16
constexpr int WL_CH = WL_N / 4;            // float4 chunks
constexpr int MC_CPT = (WL_CH + MC_NT - 1) / MC_NT;  // float4 chunks owned per thread of a CU
static_assert(WL_W3 + 2 * LD + 8 <= WL_N, "weight layout");

// Cross-GPU exchange region (one per rank, IPC-mapped by every other rank):
//   [0, 2048)    u64 flags[2 nets][XDP_MAXW ranks][CUs per network]: step id of the last share pushed
//   [2048, 2112) u64 self-test flags[XDP_MAXW ranks]
//   [4096, ...)  floats slots[2 parities][world][2 nets][WL_N]: each rank's gradient of the step
constexpr int XDP_MAXW = 8;
constexpr int XDP_TEST_OFF = 2048;     // self-test flags
constexpr int XDP_FLAGS_BYTES = 4096;  // slots start here
__host__ __device__ constexpr long long xdp_region_bytes(int world) {
  return XDP_FLAGS_BYTES + 2LL * world * 2 * WL_N * (long long)sizeof(float);
}
// byte offset of the slot that holds rank r's gradient of network `net` at step parity `par`
__host__ __device__ constexpr int xdp_slot_off(int par, int world, int r, int net) {
  return XDP_FLAGS_BYTES + ((par * world + r) * 2 + net) * WL_N * (int)sizeof(float);
}
// in `region`, the flag that CU c (of G per network) of network `net` on rank r stamps
__device__ __forceinline__ unsigned long long* xdp_flag(void* region, int net, int r, int G, int c) {
  return reinterpret_cast<unsigned long long*>(region) + (net * XDP_MAXW + r) * G + c;
}
constexpr int XDP_AUX = 17;  // sc0 | sc1: system-scope (cross-device) stores and loads

// weight-layout index -> flat torch parameters() index of this network (-1: padding).
// Branch-free (every region computed, the right one selected): per-lane branches here split the
// gathers that use it into separate basic blocks, each waiting for its own load.
template <int OUTP>
__device__ __forceinline__ int wl_to_flat(int e, int IN, int OUT, int base) {
  const int fW1 = base, fb1 = fW1 + HID * IN, fW2 = fb1 + HID, fb2 = fW2 + HID * HID, fW3 = fb2 + HID,
            fb3 = fW3 + OUT * HID;
  constexpr int WL_B3 = WL_W3 + OUTP * LD;
  const int j1 = e >> 2, k1 = e & 3;
  const int r1 = k1 < IN ? fW1 + j1 * IN + k1 : -1;
  const int r_b1 = fb1 + (e - WL_B1);
  const int q2 = e - WL_W2, j2 = q2 / LD, k2 = q2 - j2 * LD;
  const int r2 = k2 < HID ? fW2 + j2 * HID + k2 : -1;
  const int r_b2 = fb2 + (e - WL_B2);
  const int q3 = e - WL_W3, o3 = q3 / LD, k3 = q3 - o3 * LD;
  const int r3 = (o3 < OUT && k3 < HID) ? fW3 + o3 * HID + k3 : -1;
  const int o4 = e - WL_B3;
  const int r4 = (o4 >= 0 && o4 < OUT) ? fb3 + o4 : -1;
  int f = -1;
  f = e < WL_B3 + 8 ? r4 : f;
  f = e < WL_B3 ? r3 : f;
  f = e < WL_W3 ? r_b2 : f;
  f = e < WL_B2 ? r2 : f;
  f = e < WL_W2 ? r_b1 : f;
  f = e < WL_B1 ? r1 : f;
  return f;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t mc_rsrc(const void* p, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);
}
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
typedef double d2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f4 as_f4(u4v v) { return __builtin_bit_cast(f4, v); }
__device__ __forceinline__ u4v as_u4(f4 v) { return __builtin_bit_cast(u4v, v); }

// Wave-wide sums on the VALU (DPP row butterflies + lane swaps) instead of ds_bpermute shuffles:
// a fixed combination order in which every lane ends with the same bits (common.h wave_sum_dpp).
__device__ __forceinline__ float wave_sum_v(float v) { return wave_sum_dpp(v); }
__device__ __forceinline__ double wave_sum_v(double v) { return wave_sum_dpp(v); }

// torch Adam step (m, v, denom = sqrt(v)/sqrt(bc2) + eps, p -= lr/bc1 * m/denom) with the
// hardware sqrt / reciprocal (1 ulp each) instead of the IEEE-exact sequences: ~1e-7 relative
// on the update, inside the fp32 tolerance the parity tests state.
__device__ __forceinline__ void adam_update_fast(float& p, float& m, float& v, float g, float w1, float w2,
                                                 float beta2, float inv_bc2_sqrt, float neg_step, float eps) {
  m = m + w1 * (g - m);
  v = v * beta2;
  v = v + (w2 * g) * g;
  const float denom = __builtin_amdgcn_sqrtf(v) * inv_bc2_sqrt + eps;
  p = p + neg_step * (m * __builtin_amdgcn_rcpf(denom));
}

// The same update on an element pair in packed fp32 (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32: two
// elements per VALU op; per element the identical IEEE operations, so identical results), the square
// root and reciprocal per element.  The 8-CU epoch kernel's whole-network Adam is on every step's
// critical path.
typedef float f2a __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void adam_update_fast2(f2a& p, f2a& m, f2a& v, f2a g, float w1, float w2, float beta2,
                                                  float inv_bc2_sqrt, float neg_step, float eps) {
  const f2a W1 = {w1, w1}, W2 = {w2, w2}, B2 = {beta2, beta2}, IB = {inv_bc2_sqrt, inv_bc2_sqrt}, EP = {eps, eps},
            NS = {neg_step, neg_step};
  m = m + W1 * (g - m);
  v = v * B2;
  v = v + (W2 * g) * g;
  const f2a sq = {__builtin_amdgcn_sqrtf(v.x), __builtin_amdgcn_sqrtf(v.y)};
  const f2a denom = sq * IB + EP;
  const f2a rc = {__builtin_amdgcn_rcpf(denom.x), __builtin_amdgcn_rcpf(denom.y)};
  p = p + NS * (m * rc);
}

// Branch-free gather: the load is issued unconditionally (clamped index) and masked after, so
// a run of them stays in one basic block with all loads in flight (a guarded load becomes a
// branch, and the wait for its data is then placed before the next one is issued).
__device__ __forceinline__ float ld_or0(const float* p, int f) {
  const float v = p[f >= 0 ? f : 0];
  return f >= 0 ? v : 0.f;
}

// Weights -> LDS in the weight layout, and the partial-gradient buffer zeroed (padding stays 0).
// Fully unrolled so all ~19 loads per thread are in flight at once (a rolled loop waits for each load
// before the next: ~19 memory latencies, paid on every data-parallel launch).
template <int OUTP>
__device__ __forceinline__ void mc_load_weights(const MlpArgs& a, float* Wt, float* Gb, int tid, int IN, int OUT,
                                                int base) {
  constexpr int NE = (WL_N + MC_NT - 1) / MC_NT;
  float wv[NE];
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = tid + MC_NT * i;
    wv[i] = ld_or0(a.params, e < WL_N ? wl_to_flat<OUTP>(e, IN, OUT, base) : -1);
  }
#pragma unroll
  for (int i = 0; i < NE; ++i) {
    const int e = tid + MC_NT * i;
    if (e < WL_N) {
      Wt[e] = wv[i];
      Gb[e] = 0.f;
    }
  }
}

// Adam moments of the chunks this thread owns (chunk ch = tid + MC_NT * i; every CU updates the whole
// network), gathered into registers
template <int OUTP>
__device__ __forceinline__ void mc_load_moments(const MlpArgs& a, f4 (&mreg)[MC_CPT], f4 (&vreg)[MC_CPT], int tid,
                                                int IN, int OUT, int base) {
#pragma unroll
  for (int i = 0; i < MC_CPT; ++i) {
    const int ch = tid + MC_NT * i;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int f = ch < WL_CH ? wl_to_flat<OUTP>(4 * ch + q, IN, OUT, base) : -1;
      mreg[i][q] = ld_or0(a.exp_avg, f);
      vreg[i][q] = ld_or0(a.exp_avg_sq, f);
    }
  }
}

// Write back parameters and optimizer moments: the G CUs of a network hold identical copies, so CU c
// writes the chunks ch % G == c
template <int OUTP, int G>
__device__ __forceinline__ void mc_write_back(const MlpArgs& a, const float* Wt, const f4 (&mreg)[MC_CPT],
                                              const f4 (&vreg)[MC_CPT], int tid, int c, int IN, int OUT, int base) {
#pragma unroll
  for (int i = 0; i < MC_CPT; ++i) {
    const int ch = tid + MC_NT * i;
    if (ch < WL_CH && ch % G == c) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int f = wl_to_flat<OUTP>(4 * ch + q, IN, OUT, base);
        if (f >= 0) {
          a.params[f] = Wt[4 * ch + q];
          a.exp_avg[f] = mreg[i][q];
          a.exp_avg_sq[f] = vreg[i][q];
        }
      }
    }
  }
}

// Per-CU loss-statistic partials (MlpArgs::statp, through the buffer resource `str`):
// [2 nets][nmb minibatches of the launch][G CUs][4] fp64.  CU c stores minibatch k's four sums ...
template <int G>
__device__ __forceinline__ int mc_statp_off(int net, int nmb, int k, int c) {
  return ((net * nmb + k) * G + c) * 32;
}
template <int G>
__device__ __forceinline__ void mc_statp_store(__amdgpu_buffer_rsrc_t str, int net, int nmb, int k, int c,
                                               const double (&sv)[4]) {
  const u4v p0 = __builtin_bit_cast(u4v, (d2v){sv[0], sv[1]});
  const u4v p1 = __builtin_bit_cast(u4v, (d2v){sv[2], sv[3]});
  const int so = mc_statp_off<G>(net, nmb, k, c);
  __builtin_amdgcn_raw_buffer_store_b128(p0, str, so, 0, 16);
  __builtin_amdgcn_raw_buffer_store_b128(p1, str, so + 16, 0, 16);
}
// ... and at the end of the launch CU 0 sums the CUs' partials of minibatch k in CU order for its stat
// row (every CU published minibatch k's partial before the counter wait CU 0 passed for k)
template <int G>
__device__ __forceinline__ void mc_statp_sum(__amdgpu_buffer_rsrc_t str, int net, int nmb, int k, double (&sv)[4]) {
  sv[0] = sv[1] = sv[2] = sv[3] = 0.0;
  for (int cc = 0; cc < G; ++cc) {
    const int so = mc_statp_off<G>(net, nmb, k, cc);
    const auto d0 = __builtin_bit_cast(d2v, __builtin_amdgcn_raw_buffer_load_b128(str, so, 0, 16));
    const auto d1 = __builtin_bit_cast(d2v, __builtin_amdgcn_raw_buffer_load_b128(str, so + 16, 0, 16));
    sv[0] += d0[0];
    sv[1] += d0[1];
    sv[2] += d1[0];
    sv[3] += d1[1];
  }
}
