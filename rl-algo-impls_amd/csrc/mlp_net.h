// One-CU-per-network fused PPO epoch (mlp_ppo_epoch_kernel): every shape up to (in_dim, n_actions) =
// (8, 8), and the CartPole class under RAI_MLP_LAYOUT=chunk.  Included once, after ppo_row_loss.h and
// mlp_mc_common.h, inside mlp_ppo.hip's anonymous namespace (shares MlpArgs, the row loss and the helpers).
//
// The floor of this design is the f32 MFMA work of one CU per network (3 x 64x64 contractions over
// the minibatch rows), so everything else is arranged to stay off that path:
//
//  * workgroup 0 = actor, workgroup 1 = critic (no shared parameters; the only
//    coupling is clip_grad_norm_'s global norm, exchanged once per minibatch as an
//    8-byte {tag,value} granule — ~0.5 us one way, measured by tools/xchg_diag.hip);
//  * weights live in LDS (W2 also transposed for the backward), Adam moments in the
//    registers of each parameter's owning lane, W2's gradient in MFMA accumulators;
//  * the three 64-wide contractions and layer 1 run on v_mfma_f32_16x16x4_f32
//    (exact f32); the output layer is folded into layer 2's epilogue (two column-
//    half partial sums, DPP row reductions);
//  * every sum over minibatch rows (dW3, db3, db2, db1, dW1) is a per-thread partial
//    over a row slice, reduced once per minibatch through LDS (no serial row loops);
//  * the next minibatch's rows are prefetched into registers, already in the MFMA
//    A-operand layout for layer 1.
//
// The kernel is instantiated for padded (in_dim, n_actions) of (4, 2) — CartPole —
// and (8, 8); padded rows/columns carry zeros.

template <int INP, int OUTP>
struct Smem {
#ifdef RAI_STAMPS
  unsigned long long stamps[32];
  unsigned long long t_last;
#endif
  double red[NW];
  double pw[2];
  double st[16];  // loss statistics: [4 row waves][4]
  float bcast[8];
  float W1[HID][INP];  // [out j][in k]
  float b1[HID];
  float b2[HID];
  float b3[MAXOUT];
  float W2[HID][LD];   // [out j][in k]
  float W2T[HID][LD];  // [in k][out j]
  float W3[OUTP][LD];  // [out o][in k]
  float X[CH][INP];
  float H1[CH][LD];    // act(z1), later dZ1, at minibatch end: partial-gradient scratch
  float H2[CH][LD];    // act(z2), later dZ2, at minibatch end: partial-gradient scratch
  float outp[2][CH][OUTP];  // output-layer partial sums of the two column halves of H2
  float dout[CH][OUTP];
  float db3p[4][OUTP];
};

__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, float w1, float w2,
                                            float beta2, float bc2_sqrt, float neg_step, float eps) {
  m = m + w1 * (g - m);
  v = v * beta2;
  v = v + (w2 * g) * g;
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = p + neg_step * (m / denom);
}

// One network (ACTOR: the policy head; else the value head) of the fused epoch.
template <int INP, int OUTP, bool ACTOR, int RELU>
__device__ __forceinline__ void mlp_net(const MlpArgs& a, Smem<INP, OUTP>& S) {
  constexpr int net = ACTOR ? 0 : 1;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, li = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int IN = a.in_dim;
  const int NA = a.n_act;
  const int OUT = ACTOR ? NA : 1;
  constexpr int relu = RELU;  // compile-time: keeps the activation epilogues in one basic block
  RowLossHp lh = row_loss_hp(a.hp, NA);
  const float beta2 = a.ohp->beta2, adam_eps = a.ohp->eps, lr = a.ohp->lr;
  const double beta1_d = a.ohp->beta1_d, beta2_d = a.ohp->beta2_d;
  const bool grads_mode = a.grad_out != nullptr;
  const float max_grad_norm = a.ohp->max_grad_norm;

  // ---- flat parameter offsets (torch parameters() order: actor block, critic block) -------
  const int szA = HID * IN + HID + HID * HID + HID + NA * HID + NA;
  const int base = net == 0 ? 0 : szA;
  const int oW1 = base, ob1 = oW1 + HID * IN, oW2 = ob1 + HID, ob2 = oW2 + HID * HID, oW3 = ob2 + HID,
            ob3 = oW3 + OUT * HID;

  for (int e = tid; e < HID * INP; e += NT) {
    const int j = e / INP, k = e % INP;
    S.W1[j][k] = k < IN ? a.params[oW1 + j * IN + k] : 0.f;
  }
  if (tid < HID) {
    S.b1[tid] = a.params[ob1 + tid];
    S.b2[tid] = a.params[ob2 + tid];
  }
  for (int e = tid; e < HID * HID; e += NT) {
    const int j = e >> 6, k = e & 63;
    const float x = a.params[oW2 + e];
    S.W2[j][k] = x;
    S.W2T[k][j] = x;
  }
  for (int e = tid; e < OUTP * HID; e += NT) {
    const int o = e >> 6, k = e & 63;
    S.W3[o][k] = o < OUT ? a.params[oW3 + o * HID + k] : 0.f;
  }
  if (tid < MAXOUT) S.b3[tid] = tid < OUT ? a.params[ob3 + tid] : 0.f;

  // ---- ownership: W2 tile element (jt,kt) from the dW2 MFMA layout; slot A / slot B ---------
  const int jt = w >> 2, kt = w & 3;
  int w2_idx[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) w2_idx[r] = (jt * 16 + g * 4 + r) * HID + kt * 16 + li;
  // grads mode carries no optimizer state (exp_avg/exp_avg_sq are null there)
  float w2_m[4] = {0.f, 0.f, 0.f, 0.f}, w2_v[4] = {0.f, 0.f, 0.f, 0.f};
  if (!grads_mode) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      w2_m[r] = a.exp_avg[oW2 + w2_idx[r]];
      w2_v[r] = a.exp_avg_sq[oW2 + w2_idx[r]];
    }
  }
  // slot A: W3 (tid < OUT*64) | b3 (512..512+OUT) | b2 (576..639) | b1 (640..703)
  int a_flat = -1;
  if (tid < OUT * HID) a_flat = oW3 + tid;
  else if (tid >= 512 && tid < 512 + OUT) a_flat = ob3 + (tid - 512);
  else if (tid >= 576 && tid < 640) a_flat = ob2 + (tid - 576);
  else if (tid >= 640 && tid < 704) a_flat = ob1 + (tid - 640);
  // slot B: W1 (tid < 64*IN)
  const int b_flat = tid < HID * IN ? oW1 + tid : -1;
  float a_m = 0.f, a_v = 0.f, b_m = 0.f, b_v = 0.f;
  if (!grads_mode && a_flat >= 0) { a_m = a.exp_avg[a_flat]; a_v = a.exp_avg_sq[a_flat]; }
  if (!grads_mode && b_flat >= 0) { b_m = a.exp_avg[b_flat]; b_v = a.exp_avg_sq[b_flat]; }

  const int B = a.batch;
  const int64_t n_rows = a.n_rows;
  const int nmb_total = (int)((n_rows + B - 1) / B);
  const int mb_begin = a.mb_begin;
  const int mb_end = min(nmb_total, a.mb_begin + a.mb_count);
  const int nmb = mb_end - mb_begin;
  const int64_t step0 = a.state->opt_step;
  const int stat0 = a.state->stat_index;
  const int norm0 = a.state->norm_index;
  lh.pi_coef = a.state->pi_coef_zero ? 0.f : 1.f;

  // ---- per-minibatch inputs, prefetched into registers one minibatch ahead ------------------
  // thread t < rows: row t's (action, old logp, adv | old value, return);
  // px[c][q]: X[c*CH + (w>>1)*16 + li][4q + g] = the layer-1 MFMA A operand of chunk c
  constexpr int NQ = INP / 4;
  int r_act = 0;
  float r_a = 0.f, r_b = 0.f, r_c = 0.f, r_d = 1.f;
  float px[2][NQ];
  auto prefetch = [&](int mb) {
    const int64_t row0 = (int64_t)mb * B;
    const int rows = (int)min((int64_t)B, n_rows - row0);
    if (tid < rows) {
      const int64_t r = row0 + tid;
      if (ACTOR) {
        r_act = (int)a.actions[r];
        r_a = a.old_logp[r];
        r_b = a.adv[r];
      } else {
        r_a = a.old_values[r];
        r_b = a.ret[r];
      }
    }
    if (ACTOR) {
      r_c = a.moments[2 * mb];
      r_d = a.moments[2 * mb + 1];
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int s = c * CH + (w >> 1) * 16 + li;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int k = 4 * q + g;
        px[c][q] = (s < rows && k < IN) ? a.obs[(row0 + s) * IN + k] : 0.f;
      }
    }
  };
  prefetch(mb_begin);
  if (tid == 0) {  // running powers beta^step (bias corrections), advanced once per minibatch
    S.pw[0] = ipow(beta1_d, step0);
    S.pw[1] = ipow(beta2_d, step0);
  }
#ifdef RAI_STAMPS
  if (tid < 32) S.stamps[tid] = 0;
  if (tid == 0) S.t_last = __builtin_amdgcn_s_memtime();
#endif
  lds_barrier();

  for (int mb = mb_begin; mb < mb_end; ++mb) {
    const int64_t row0 = (int64_t)mb * B;
    const int rows = (int)min((int64_t)B, n_rows - row0);
    // take this minibatch's inputs out of the prefetch registers
    const int c_act = r_act;
    const float c_a = r_a, c_b = r_b;
    float cx[2][NQ];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < NQ; ++q) cx[c][q] = px[c][q];
    const float amean = r_c, aden = r_d;
    if (mb + 1 < mb_end) prefetch(mb + 1);
    lh.invB = 1.f / (float)(rows * a.world);

    // per-thread partial gradients over this minibatch's rows
    f4 gw2 = {0.f, 0.f, 0.f, 0.f};   // dW2 tile (MFMA accumulator)
    float p_w3[OUTP], p_b2 = 0.f;    // B1 layout: column k = lane, rows w + 16 i
    float p_b1[2] = {0.f, 0.f};      // B3 layout: columns k0, k0 + 16, rows of tile (w>>1)
    float p_w1 = 0.f;                // B4 layout: (j = lane, k, row slice)
    float my_dout[OUTP];             // this thread's row (L layout), for db3
    float st[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < OUTP; ++o) { p_w3[o] = 0.f; my_dout[o] = 0.f; }

    const int nch = (rows + CH - 1) / CH;
    for (int c = 0; c < nch; ++c) {
      const int crows = min(CH, rows - c * CH);
      // ---- F1: layer 1 on MFMA (K = in_dim padded to 4/8), act -> H1; X -> LDS for dW1 ----------
      {
        RELANE();
        const int mt = w >> 1, ntb = (w & 1) * 2;
        f4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
          const float av = c == 0 ? cx[0][q] : cx[1][q];
          const float b0 = S.W1[ntb * 16 + li][4 * q + g];
          const float b1 = S.W1[(ntb + 1) * 16 + li][4 * q + g];
          z0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, z0, 0, 0, 0);
          z1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, z1, 0, 0, 0);
          if ((w & 1) == 0) S.X[mt * 16 + li][4 * q + g] = av;
        }
        const int j0 = ntb * 16 + li;
        const float bb0 = S.b1[j0], bb1 = S.b1[j0 + 16];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s = mt * 16 + g * 4 + r;
          S.H1[s][j0] = act_f(relu, z0[r] + bb0);
          S.H1[s][j0 + 16] = act_f(relu, z1[r] + bb1);
        }
      }
      lds_barrier();
      STAMP(1);
      // ---- F2: layer 2 on MFMA, act -> H2; output layer folded into the epilogue -----------------
      {
        RELANE();
        const int mt = w >> 1, nt0 = (w & 1) * 2;
        f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 16; kk += 2) {
          const int kq = kmap(g, kk);
          const f2 av = *reinterpret_cast<const f2*>(&S.H1[mt * 16 + li][kq]);
          const f2 b0 = *reinterpret_cast<const f2*>(&S.W2[nt0 * 16 + li][kq]);
          const f2 b1 = *reinterpret_cast<const f2*>(&S.W2[(nt0 + 1) * 16 + li][kq]);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b0.x, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b1.x, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b0.y, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b1.y, acc1, 0, 0, 0);
        }
        const int j0 = nt0 * 16 + li;
        const float bb0 = S.b2[j0], bb1 = S.b2[j0 + 16];
        float w3a[OUTP], w3b[OUTP];
#pragma unroll
        for (int o = 0; o < OUTP; ++o) {
          w3a[o] = S.W3[o][j0];
          w3b[o] = S.W3[o][j0 + 16];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s = mt * 16 + g * 4 + r;
          const float h0 = act_f(relu, acc0[r] + bb0);
          const float h1 = act_f(relu, acc1[r] + bb1);
          S.H2[s][j0] = h0;
          S.H2[s][j0 + 16] = h1;
#pragma unroll
          for (int o = 0; o < OUTP; ++o) {
            const float part = row_sum16(fmaf(h1, w3b[o], h0 * w3a[o]));
            if (li == ((r * OUTP + o) & 15)) S.outp[w & 1][s][o] = part;
          }
        }
      }
      lds_barrier();
      STAMP(2);
      // ---- L: per-row loss gradient w.r.t. the head outputs (ppo.py:326-371 semantics; autograd
      //      tie rules of min/max and closed-interval clamp: ppo_terms.h) ---------------------------
      {
        RELANE();
        const int s = tid - c * CH;
        if (s >= 0 && s < CH) {
          float d[OUTP];
#pragma unroll
          for (int o = 0; o < OUTP; ++o) d[o] = 0.f;
          if (s < crows) {
            float z[OUTP];
#pragma unroll
            for (int o = 0; o < OUTP; ++o) z[o] = (S.outp[0][s][o] + S.outp[1][s][o]) + S.b3[o];
            float sr[4] = {0.f, 0.f, 0.f, 0.f};
            ppo_row_loss<OUTP, ACTOR>(z, lh, c_act, c_a, c_b, ACTOR ? (c_b - amean) / aden : 0.f, d, sr);
#pragma unroll
            for (int i = 0; i < (ACTOR ? 4 : 2); ++i) st[i] += sr[i];
          }
#pragma unroll
          for (int o = 0; o < OUTP; ++o) {
            S.dout[s][o] = d[o];
            my_dout[o] = d[o];
          }
        }
      }
      lds_barrier();
      STAMP(3);
      // ---- B1: dZ2 = (dout . W3) * act'(H2) in place over H2; dW3, db2 partials (column k) ------
      {
        RELANE();
        const int k = lane;
        float w3[OUTP];
#pragma unroll
        for (int o = 0; o < OUTP; ++o) w3[o] = S.W3[o][k];
#pragma unroll
        for (int i = 0; i < CH / NW; ++i) {
          const int s = w + NW * i;
          const float h = S.H2[s][k];
          float dh = 0.f;
#pragma unroll
          for (int o = 0; o < OUTP; ++o) {
            const float dv = S.dout[s][o];
            dh = fmaf(dv, w3[o], dh);
            p_w3[o] = fmaf(dv, h, p_w3[o]);
          }
          const float dz = dh * act_d(relu, h);
          p_b2 += dz;
          S.H2[s][k] = dz;
        }
      }
      lds_barrier();
      STAMP(4);
      // ---- B2: dW2 += dZ2^T H1 (accumulators persist over chunks), dH1 = dZ2 W2 (held) ---------
      f4 h0 = {0.f, 0.f, 0.f, 0.f}, h1 = {0.f, 0.f, 0.f, 0.f};
      {
        RELANE();
#pragma unroll 8
        for (int kk = 0; kk < 32; ++kk) {
          const int s = smap(g, kk);
          const int jt = w >> 2, kt = w & 3;
          gw2 = __builtin_amdgcn_mfma_f32_16x16x4f32(S.H2[s][jt * 16 + li], S.H1[s][kt * 16 + li], gw2, 0, 0, 0);
        }
        const int mt = w >> 1, nt0 = (w & 1) * 2;
#pragma unroll
        for (int kk = 0; kk < 16; kk += 2) {
          const int kq = kmap(g, kk);
          const f2 av = *reinterpret_cast<const f2*>(&S.H2[mt * 16 + li][kq]);
          const f2 b0 = *reinterpret_cast<const f2*>(&S.W2T[nt0 * 16 + li][kq]);
          const f2 b1 = *reinterpret_cast<const f2*>(&S.W2T[(nt0 + 1) * 16 + li][kq]);
          h0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b0.x, h0, 0, 0, 0);
          h1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, b1.x, h1, 0, 0, 0);
          h0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b0.y, h0, 0, 0, 0);
          h1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, b1.y, h1, 0, 0, 0);
        }
      }
      lds_barrier();
      STAMP(5);
      // ---- B3: dZ1 = dH1 * act'(H1) in place over H1; db1 partials -------------------------------
      {
        RELANE();
        const int mt = w >> 1, k0 = (w & 1) * 32 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s = mt * 16 + g * 4 + r;
          const float da = h0[r] * act_d(relu, S.H1[s][k0]);
          const float db = h1[r] * act_d(relu, S.H1[s][k0 + 16]);
          S.H1[s][k0] = da;
          S.H1[s][k0 + 16] = db;
          p_b1[0] += da;
          p_b1[1] += db;
        }
      }
      lds_barrier();
      STAMP(6);
      // ---- B4: dW1 partial over a row slice (j = lane, k = w % INP, slice = w / INP) -------------
      {
        RELANE();
        constexpr int NSL = NW / INP, RS = CH / NSL;
        const int k = w % INP, sl = w / INP;
        float acc = 0.f;
#pragma unroll 8
        for (int i = 0; i < RS; ++i) {
          const int s = sl * RS + i;
          acc = fmaf(S.H1[s][lane], S.X[s][k], acc);
        }
        p_w1 += acc;
      }
      lds_barrier();
      STAMP(7);
    }

    // ---- E1: per-thread partials -> LDS (H1/H2 are free now) -------------------------------------
    float* R3 = &S.H2[0][0];           // [NW][OUTP][64]
    float* Rb2 = &S.H1[0][0];          // [NW][64]
    float* Rb1 = Rb2 + NW * HID;       // [8 row tiles][64]
    float* RW1 = Rb1 + 8 * HID;        // [NW / INP slices][INP][64]
    {
      RELANE();
#pragma unroll
      for (int o = 0; o < OUTP; ++o) R3[(w * OUTP + o) * HID + lane] = p_w3[o];
      Rb2[w * HID + lane] = p_b2;
      float b1a = p_b1[0] + __shfl_xor(p_b1[0], 16, 64);
      float b1b = p_b1[1] + __shfl_xor(p_b1[1], 16, 64);
      b1a += __shfl_xor(b1a, 32, 64);
      b1b += __shfl_xor(b1b, 32, 64);
      if (g == 0) {
        const int mt = w >> 1, k0 = (w & 1) * 32 + li;
        Rb1[mt * HID + k0] = b1a;
        Rb1[mt * HID + k0 + 16] = b1b;
      }
      RW1[((w / INP) * INP + (w % INP)) * HID + lane] = p_w1;
      if (w < 4) {  // rows live in threads 0..255: db3 and the loss statistics
#pragma unroll
        for (int o = 0; o < OUTP; ++o) {
          const float t = wave_sum(my_dout[o]);
          if (lane == 0) S.db3p[w][o] = t;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double t = wave_sum((double)st[i]);
          if (lane == 0) S.st[w * 4 + i] = t;
        }
      }
    }
    lds_barrier();
    STAMP(8);
    // ---- E2: owners sum partials in fixed order; squared norm of this network's gradient ----------
    float ga = 0.f, gb = 0.f;
    {
      RELANE();
      if (tid < OUT * HID) {
        const int o = tid >> 6, k = tid & 63;
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < NW; ++q) t += R3[(q * OUTP + o) * HID + k];
        ga = t;
      } else if (tid >= 512 && tid < 512 + OUT) {
        const int o = tid - 512;
        ga = ((S.db3p[0][o] + S.db3p[1][o]) + S.db3p[2][o]) + S.db3p[3][o];
      } else if (tid >= 576 && tid < 640) {
        const int j = tid - 576;
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < NW; ++q) t += Rb2[q * HID + j];
        ga = t;
      } else if (tid >= 640 && tid < 704) {
        const int j = tid - 640;
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) t += Rb1[q * HID + j];
        ga = t;
      }
      if (b_flat >= 0) {
        const int j = tid / IN, k = tid % IN;
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < NW / INP; ++q) t += RW1[(q * INP + k) * HID + j];
        gb = t;
      }
      double ss = (double)gw2.x * gw2.x + (double)gw2.y * gw2.y + (double)gw2.z * gw2.z + (double)gw2.w * gw2.w;
      if (a_flat >= 0) ss += (double)ga * ga;
      if (b_flat >= 0) ss += (double)gb * gb;
      ss = wave_sum(ss);
      if (lane == 0) S.red[w] = ss;
      if (grads_mode) {
        // raw gradients out (same flat indices as the parameters)
#pragma unroll
        for (int r = 0; r < 4; ++r) a.grad_out[oW2 + w2_idx[r]] = gw2[r];
        if (a_flat >= 0) a.grad_out[a_flat] = ga;
        if (b_flat >= 0) a.grad_out[b_flat] = gb;
      }
    }
    lds_barrier();
    STAMP(9);
    // ---- E3: stats row, grad-norm exchange with the other network, bias corrections ---------------
    if (tid == 0) {
      double ssum = 0.0;
      for (int q = 0; q < NW; ++q) ssum += S.red[q];
      const double* stp = S.st;
      double sv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) sv[i] = ((stp[0 * 4 + i] + stp[1 * 4 + i]) + stp[2 * 4 + i]) + stp[3 * 4 + i];
      const int srow = stat0 + (mb - mb_begin);
      if (a.stats && srow < a.max_stats)
        stat_row_write<ACTOR>(a.stats + (int64_t)srow * RAI_STAT_STRIDE, sv, rows, a.world, lh);
      if (!grads_mode) {
        const float mine = (float)ssum;
        const unsigned tag = (unsigned)(mb + 1);
        const int par = mb & 1;
        const unsigned long long gr = ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(mine);
        __hip_atomic_store(&a.xchg[net * 2 + par], gr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        float other = 0.f;
        unsigned long long spins = 0;
        for (;;) {
          const unsigned long long x =
              __hip_atomic_load(&a.xchg[(1 - net) * 2 + par], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if ((unsigned)(x >> 32) == tag) { other = __uint_as_float((unsigned)x); break; }
          if (++spins > (1ull << 26)) { atomicExch(a.err, 1); break; }  // bounded: never hangs
          __builtin_amdgcn_s_sleep(1);
        }
        S.bcast[0] = net == 0 ? mine : other;
        S.bcast[1] = net == 0 ? other : mine;
        S.pw[0] *= beta1_d;
        S.pw[1] *= beta2_d;
        const double bc1 = 1.0 - S.pw[0];
        const double bc2 = 1.0 - S.pw[1];
        S.bcast[2] = (float)sqrt(bc2);
        S.bcast[3] = (float)(-((double)lr / bc1));
      }
    }
    lds_barrier();
    STAMP(10);
    if (grads_mode) continue;
    const float total_norm = (float)sqrt((double)S.bcast[0] + (double)S.bcast[1]);
    const float coef = clip_coef(max_grad_norm, total_norm);
    const float bc2_sqrt = S.bcast[2], neg_step = S.bcast[3];
    const float w1 = (float)(1.0 - beta1_d), w2 = (float)(1.0 - beta2_d);

    // ---- E4: Adam on owned parameters; refresh the LDS copies --------------------------------------
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = w2_idx[r] >> 6, k = w2_idx[r] & 63;
      float p = S.W2[j][k];
      adam_update(p, w2_m[r], w2_v[r], gw2[r] * coef, w1, w2, beta2, bc2_sqrt, neg_step, adam_eps);
      S.W2[j][k] = p;
      S.W2T[k][j] = p;
    }
    if (a_flat >= 0) {
      float* slot;
      if (tid < OUT * HID) slot = &S.W3[tid >> 6][tid & 63];
      else if (tid < 576) slot = &S.b3[tid - 512];
      else if (tid < 640) slot = &S.b2[tid - 576];
      else slot = &S.b1[tid - 640];
      float p = *slot;
      adam_update(p, a_m, a_v, ga * coef, w1, w2, beta2, bc2_sqrt, neg_step, adam_eps);
      *slot = p;
    }
    if (b_flat >= 0) {
      const int j = tid / IN, k = tid % IN;
      float p = S.W1[j][k];
      adam_update(p, b_m, b_v, gb * coef, w1, w2, beta2, bc2_sqrt, neg_step, adam_eps);
      S.W1[j][k] = p;
    }
    if (tid == 0) {
      if (ACTOR && a.norms && norm0 + (mb - mb_begin) < a.max_norms) a.norms[norm0 + (mb - mb_begin)] = total_norm;
    }
    lds_barrier();
    STAMP(11);
  }

  // ---- write back parameters and optimizer moments (torch parameter order) -----------------------
  if (!grads_mode) {
    int t2 = tid;
    asm volatile("" : "+v"(t2));
    const int lane2 = t2 & 63, w_2 = t2 >> 6, g2 = lane2 >> 4, li2 = lane2 & 15;
    const int jt2 = w_2 >> 2, kt2 = w_2 & 3;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = jt2 * 16 + g2 * 4 + r, k = kt2 * 16 + li2;
      const int idx = oW2 + j * HID + k;
      a.params[idx] = S.W2[j][k];
      a.exp_avg[idx] = w2_m[r];
      a.exp_avg_sq[idx] = w2_v[r];
    }
    int af = -1;
    float p = 0.f;
    if (t2 < OUT * HID) { af = oW3 + t2; p = S.W3[t2 >> 6][t2 & 63]; }
    else if (t2 >= 512 && t2 < 512 + OUT) { af = ob3 + (t2 - 512); p = S.b3[t2 - 512]; }
    else if (t2 >= 576 && t2 < 640) { af = ob2 + (t2 - 576); p = S.b2[t2 - 576]; }
    else if (t2 >= 640 && t2 < 704) { af = ob1 + (t2 - 640); p = S.b1[t2 - 640]; }
    if (af >= 0) {
      a.params[af] = p;
      a.exp_avg[af] = a_m;
      a.exp_avg_sq[af] = a_v;
    }
    if (t2 < HID * IN) {
      a.params[oW1 + t2] = S.W1[t2 / IN][t2 % IN];
      a.exp_avg[oW1 + t2] = b_m;
      a.exp_avg_sq[oW1 + t2] = b_v;
    }
  }
#ifdef RAI_STAMPS
  if (tid < 32) g_stamps[net][tid] = S.stamps[tid];
#endif
  // grads mode has no per-minibatch exchange, so the actor must not advance the shared
  // stat_index before the critic has read it: the critic posts a done flag, the actor waits.
  if (grads_mode && tid == 0) {
    if (!ACTOR) {
      __hip_atomic_store(&a.xchg[4], 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      unsigned long long spins = 0;
      while (__hip_atomic_load(&a.xchg[4], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == 0ull) {
        if (++spins > (1ull << 26)) { atomicExch(a.err, 1); break; }
        __builtin_amdgcn_s_sleep(1);
      }
    }
  }
  if (ACTOR && tid == 0) {
    a.state->stat_index = stat0 + nmb;
    if (!grads_mode) {
      a.state->opt_step = step0 + nmb;
      a.state->norm_index = norm0 + nmb;
    }
  }
}

template <int INP, int NAP, int RELU>
__global__ __launch_bounds__(NT) void mlp_ppo_epoch_kernel(const MlpArgs a) {
  static_assert(sizeof(Smem<INP, NAP>) <= 160 * 1024, "LDS budget");
  __shared__ __attribute__((aligned(16))) unsigned char smem_raw[sizeof(Smem<INP, NAP>)];
  if (blockIdx.x == 0) mlp_net<INP, NAP, true, RELU>(a, *reinterpret_cast<Smem<INP, NAP>*>(smem_raw));
  else mlp_net<INP, 1, false, RELU>(a, *reinterpret_cast<Smem<INP, 1>*>(smem_raw));
}
