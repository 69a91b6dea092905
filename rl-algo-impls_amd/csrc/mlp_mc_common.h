// Shared by the multi-CU fused PPO epoch kernels (mlp_mc.h: 4 CUs per network; mlp_mc8.h: 8 or 16):
// the weight layout of LDS / partial-gradient buffers / exchange slots, the cross-GPU exchange
// region, and the small device helpers both kernels use.  Included once, inside mlp_ppo.hip's
// anonymous namespace, before mlp_mc.h and mlp_mc8.h (uses HID, LD, f4 and common.h).

// Weight layout shared by LDS, the partial-gradient buffers and the exchange slots (floats).
constexpr int WL_W1 = 0;                   // [64][4]
constexpr int WL_B1 = WL_W1 + HID * 4;     // [64]
constexpr int WL_W2 = WL_B1 + HID;         // [64][LD]
constexpr int WL_B2 = WL_W2 + HID * LD;    // [64]
constexpr int WL_W3 = WL_B2 + HID;         // [OUTP][LD]
constexpr int WL_N = 4752;                 // >= WL_W3 + 2 * LD + 8, multiple of 16
constexpr int WL_CH = WL_N / 4;            // float4 chunks
// float4 chunks owned per thread of a 256-thread CU (MC_NT and M8_NT)
constexpr int MC_CPT = (WL_CH + 256 - 1) / 256;
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
