// ouz_policy_rollout_lstm: the fused rollout with the recurrent actor in the loop: LSTMActor's
// 13 -> 512 -> 256 tanh trunk, LSTM(256, 128) and 128 -> 4 mean head (learners/models.py).  Included after
// quad_policy.h, whose env side it takes unchanged (env_load once, K x (sample -> env_core -> emit), env_store once,
// the fused statistics) together with pol_corrupt, pol_put_input, pol_sample, pol_norm and the RNG_POLICY eps key.
//
// One workgroup of four waves per 64-env tile; the waves meet at __syncthreads() alone, eight barriers per step,
// reached by every wave of every workgroup K times (K is a kernel argument; a partial tile's idle lanes hold zero
// input rows and store nothing).
//   step k:  [B1] layer 1, units 0..255 (thread t owns units t and 256 + t; the tile's input rows from LDS) -> s_a
//            [B2] layer 2's first half on v_mfma_f32_16x16x4_f32 (wave w owns units 64 w .. 64 w + 63, all 64 rows)
//            [B3] layer 1, units 256..511 -> s_a
//            [B4] layer 2's second half into the same accumulators
//            [B5] bias + tanh of the accumulators -> s_a (h2)
//            [B6] gates: wave w owns hidden units 32 w .. 32 w + 31, two 16-unit blocks, for each the four gate tiles
//                 of all 64 rows, so a lane holds i, f, g, o of its (row, unit) elements (the sequence kernels'
//                 ownership); h2 W_ih^T then h_prev W_hh^T into accumulators that start at b_ih + b_hh; the cell;
//                 h' into the other h buffer (double-buffered by step parity), c stays in registers
//            [B7] head: thread t = 4 row + a, one dot product of 128
//            [B8] wave 0, the state wave: sample, log-prob, stores, env step, outputs, the corruption, the next
//                 policy input and the next keep flag into LDS; waves 1-3 wait at the next step's B1.
// The carry of a row is zeroed where it is read (a select on the row's keep flag), never by arithmetic, so a reset
// carry is exactly the zero carry.  Every output element is a sum over k in one fixed order that does not depend on
// the row's place in the tile or on the shard.
#pragma once

namespace ouz {

constexpr int kLstmT1 = 512;            // trunk layer 1 width
constexpr int kLstmT2 = 256;            // trunk layer 2 width == the LSTM's input (== kPolH: s_a's row)
constexpr int kLstmH = 128;             // hidden size
constexpr int kLstmHLd = kLstmH + 4;    // carry row stride in LDS, floats
static_assert(kLstmT2 == kPolH && kLstmT1 == 2 * kPolBlock, "the halves of layer 1 and the activation row");

struct LstmArgs {
  const float *w_ih, *w_hh, *b_ih, *b_hh;
  const float *h_in, *c_in;
  const float* done_in0;        // the done of step 0's input as f32, or
  const int64_t* reset_in0;     // as a stored reset row (a later chunk of one call)
  float *h_out, *c_out;         // may be h_in / c_in: a workgroup reads its rows first and writes them last
};

// learner_kernels.hip's fsigm (the sequence kernels' sigmoid), restated for this unit as pol_tanh restates ftanh
__device__ __forceinline__ float pol_sigm(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}
__device__ __forceinline__ pf4 pol_mfma4(pf4 a, pf4 b, pf4 c) {
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, c, 0, 0, 0);
}

template <int TASK>
__global__ void __launch_bounds__(kPolBlock) quad_lstm_policy_rollout_kernel(StepArgs a, RolloutArgs r, PolicyArgs p,
                                                                             LstmArgs q) {
  constexpr int CTRL = task_ctrl(TASK), TGT = task_tgt(TASK);
  constexpr unsigned FORM = F_MULTI;   // the general one-wave rollout form, as quad_policy_rollout_kernel
  static_assert(CTRL == CTRL_RL, "the tasks whose step takes the policy's action");
  __shared__ float s_a[64 * kPolLd];            // layer 1's activations, one 256-unit half at a time; then h2
  __shared__ float s_hp[2][64 * kLstmHLd];      // h entering the step (unmasked) and h leaving it, by step parity
  __shared__ float s_x[64 * kPolXLd];           // policy input rows
  __shared__ float s_wh[OUZ_NUM_ACT * kLstmH];  // the head's weights
  __shared__ float s_mean[64 * OUZ_NUM_ACT];
  __shared__ float s_keep[64];                  // 0: the row's carry is zeroed before the step
  __shared__ float4 s_obs4[64 * OUZ_NUM_OBS / 4];   // emit's staging (the state wave's)
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, l16 = lane & 15u, g4 = lane >> 4;
  const int K = r.K;
  const size_t n = (size_t)a.n;
  const size_t tile0 = (size_t)blockIdx.x * 64u;

  // ---- launch prologue: weights that stay on chip, the carry, the state, the first input ----
  if (t < (uint32_t)(OUZ_NUM_ACT * kLstmH / 4))
    *reinterpret_cast<pf4*>(s_wh + 4 * t) = *reinterpret_cast<const pf4*>(p.w3 + 4 * t);
  float w1r[2][OUZ_NUM_OBS], b1t[2];
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
    for (int j = 0; j < OUZ_NUM_OBS; ++j) w1r[hf][j] = p.w1[(size_t)(kPolBlock * hf + t) * OUZ_NUM_OBS + j];
    b1t[hf] = p.b1[kPolBlock * hf + t];
  }
  for (uint32_t j = t; j < 64u * kPolXLd; j += kPolBlock) s_x[j] = 0.0f;   // (the three pad columns stay zero)
  for (uint32_t e = t; e < 64u * (kLstmH / 4); e += kPolBlock) {
    const uint32_t row = e / (kLstmH / 4), j4 = e % (kLstmH / 4);
    const size_t gi = tile0 + row;
    const pf4 v = gi < n ? *reinterpret_cast<const pf4*>(q.h_in + gi * kLstmH + 4u * j4) : pf4{0.0f, 0.0f, 0.0f, 0.0f};
    *reinterpret_cast<pf4*>(&s_hp[0][row * kLstmHLd + 4u * j4]) = v;
  }
  if (t < 64u) {
    const size_t gi = tile0 + t;
    bool done = false;
    if (gi < n) done = q.reset_in0 ? q.reset_in0[gi] != 0 : q.done_in0[gi] != 0.0f;
    s_keep[t] = done ? 0.0f : 1.0f;
  }
  // this lane's cell state: rows 16 et + (l & 15), units 32 wave + 16 jb + 4 (l >> 4) + 0..3
  pf4 c[2][4];
#pragma unroll
  for (int jb = 0; jb < 2; ++jb)
#pragma unroll
    for (int et = 0; et < 4; ++et) {
      const size_t gi = tile0 + 16u * et + l16;
      c[jb][et] = gi < n ? *reinterpret_cast<const pf4*>(q.c_in + gi * kLstmH + 32u * wave + 16u * jb + 4u * g4)
                         : pf4{0.0f, 0.0f, 0.0f, 0.0f};
    }
  __syncthreads();

  // the state wave's lane: slot i == env e (identity layout), as run_env
  const int i = (int)(blockIdx.x * 64u + lane), e = i;
  const bool valid = wave == 0u && i < a.n;
  const TaskParams& tp = a.tp[tp_slot(TASK)];
  const uint32_t gid = a.env_offset + (uint32_t)e;
  const int sm = r.stats.mode;
  LaneStats ls{0.0, 0.0, 0.0};
  EnvRegs<CTRL, TGT> S;
  float ep_sum_old = 0.0f;
  int32_t ep_cnt_old = 0, ep_len_old = 0;
  float lsd[OUZ_NUM_ACT];
#pragma unroll
  for (int j = 0; j < OUZ_NUM_ACT; ++j) lsd[j] = p.logstd[j];
  if (wave == 0u) {
    S.T = tile_of(a, i);
    if (sm && valid) {
      ep_sum_old = ld(S.T, OUZ_F_EP_SUM);
      ep_cnt_old = ldi(S.T, OUZ_I_EP_CNT);
      ep_len_old = ldi(S.T, OUZ_I_EP_LEN);
    }
    if (valid) env_load<CTRL, TGT, load_form(FORM)>(a, e, tp, S, r.ctx[0].actions);
    float x0[OUZ_NUM_OBS];
#pragma unroll
    for (int j = 0; j < OUZ_NUM_OBS; ++j) x0[j] = valid ? p.in0[(size_t)i * OUZ_NUM_OBS + j] : 0.0f;
    pol_put_input(p, s_x, lane, valid, x0);
    __builtin_amdgcn_s_waitcnt(kWaitVmcnt0);   // run_env: the state loads drain before the step loop
  }

  for (int k = 0; k < K; ++k) {
    const int cur = k & 1, nxt = cur ^ 1;
    __syncthreads();   // B1: the input rows and keep flags of step k
    // ---- trunk.  Layer 1: h1[row][u] = tanh(b1[u] + sum_j x[row][j] w1[u][j]), j ascending, one 256-unit half at a
    // time into s_a.  Layer 2, transposed as the sequence kernels do: out^T = W2 h1^T, the weight tile the MFMA's A
    // operand (unit l & 15 of the tile), the activation tile its B operand (row l & 15), so lane l holds units
    // 4 (l >> 4) + 0..3 of row l & 15.  k order within a half: lane group l >> 4 walks k = 64 (l >> 4) + 4 s .. + 3,
    // so four consecutive MFMA steps take one 16-byte load per operand; the first half's 256 k before the second's. ----
    pf4 acc2[4][4];
#pragma unroll
    for (int ut = 0; ut < 4; ++ut)
#pragma unroll
      for (int et = 0; et < 4; ++et) acc2[ut][et] = pf4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      if (hf) __syncthreads();   // B3: every wave has read the first half
      for (int row = 0; row < 64; ++row) {
        const pf4* xr = reinterpret_cast<const pf4*>(s_x + row * kPolXLd);
        const pf4 x0 = xr[0], x1 = xr[1], x2 = xr[2], x3 = xr[3];
        float acc = b1t[hf];
        acc = fmaf(x0.x, w1r[hf][0], acc); acc = fmaf(x0.y, w1r[hf][1], acc); acc = fmaf(x0.z, w1r[hf][2], acc);
        acc = fmaf(x0.w, w1r[hf][3], acc); acc = fmaf(x1.x, w1r[hf][4], acc); acc = fmaf(x1.y, w1r[hf][5], acc);
        acc = fmaf(x1.z, w1r[hf][6], acc); acc = fmaf(x1.w, w1r[hf][7], acc); acc = fmaf(x2.x, w1r[hf][8], acc);
        acc = fmaf(x2.y, w1r[hf][9], acc); acc = fmaf(x2.z, w1r[hf][10], acc); acc = fmaf(x2.w, w1r[hf][11], acc);
        acc = fmaf(x3.x, w1r[hf][12], acc);
        s_a[row * kPolLd + t] = pol_tanh(acc);
      }
      __syncthreads();   // B2 / B4
      const float* wbase = p.w2 + (size_t)(64u * wave + l16) * kLstmT1 + kPolH * hf + 64u * g4;
      const float* hbase = s_a + l16 * kPolLd + 64u * g4;
#pragma unroll 2
      for (int s = 0; s < 16; ++s) {
        pf4 wa[4], hb[4];
#pragma unroll
        for (int ut = 0; ut < 4; ++ut) wa[ut] = *reinterpret_cast<const pf4*>(wbase + (size_t)(16 * ut) * kLstmT1 + 4 * s);
#pragma unroll
        for (int et = 0; et < 4; ++et) hb[et] = *reinterpret_cast<const pf4*>(hbase + (16 * et) * kPolLd + 4 * s);
#pragma unroll
        for (int ut = 0; ut < 4; ++ut)
#pragma unroll
          for (int et = 0; et < 4; ++et) acc2[ut][et] = pol_mfma4(wa[ut], hb[et], acc2[ut][et]);
      }
    }
    __syncthreads();   // B5: every wave has read h1
#pragma unroll
    for (int ut = 0; ut < 4; ++ut) {
      const uint32_t unit0 = 64u * wave + 16u * ut + 4u * g4;
      const pf4 b2v = *reinterpret_cast<const pf4*>(p.b2 + unit0);
#pragma unroll
      for (int et = 0; et < 4; ++et) {
        const pf4 v = acc2[ut][et] + b2v;
        *reinterpret_cast<pf4*>(s_a + (16u * et + l16) * kPolLd + unit0) =
            pf4{pol_tanh(v.x), pol_tanh(v.y), pol_tanh(v.z), pol_tanh(v.w)};
      }
    }
    __syncthreads();   // B6: h2
    // ---- gates and cell.  Per 16-unit block jb: gate tile g covers gate rows 128 g + 32 wave + 16 jb + 0..15 (the A
    // operand), all 64 rows (four B tiles).  The accumulators start at b_ih + b_hh (one f32 add, as get_states forms
    // the bias), take h2 W_ih^T (k = 64 (l >> 4) + 4 s ..) and then h W_hh^T (k = 32 (l >> 4) + 4 s ..). ----
    {
      bool kp[4];
#pragma unroll
      for (int et = 0; et < 4; ++et) kp[et] = s_keep[16u * et + l16] != 0.0f;
      const float* h_cur = s_hp[cur];
      float* h_nxt = s_hp[nxt];
#pragma unroll
      for (int jb = 0; jb < 2; ++jb) {
        const uint32_t u0 = 32u * wave + 16u * jb;
        pf4 acc[4][4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const uint32_t gr = (uint32_t)kLstmH * g + u0 + 4u * g4;
          const pf4 bg = *reinterpret_cast<const pf4*>(q.b_ih + gr) + *reinterpret_cast<const pf4*>(q.b_hh + gr);
#pragma unroll
          for (int et = 0; et < 4; ++et) acc[g][et] = bg;
        }
        {
          const float* wbase = q.w_ih + (size_t)(u0 + l16) * kLstmT2 + 64u * g4;
          const float* hbase = s_a + l16 * kPolLd + 64u * g4;
#pragma unroll 2
          for (int s = 0; s < 16; ++s) {
            pf4 wa[4], hb[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
              wa[g] = *reinterpret_cast<const pf4*>(wbase + (size_t)(kLstmH * g) * kLstmT2 + 4 * s);
#pragma unroll
            for (int et = 0; et < 4; ++et) hb[et] = *reinterpret_cast<const pf4*>(hbase + (16 * et) * kPolLd + 4 * s);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
              for (int et = 0; et < 4; ++et) acc[g][et] = pol_mfma4(wa[g], hb[et], acc[g][et]);
          }
        }
        {
          const float* wbase = q.w_hh + (size_t)(u0 + l16) * kLstmH + 32u * g4;
          const float* hbase = h_cur + l16 * kLstmHLd + 32u * g4;
#pragma unroll 2
          for (int s = 0; s < 8; ++s) {
            pf4 wa[4], hb[4];
#pragma unroll
            for (int g = 0; g < 4; ++g)
              wa[g] = *reinterpret_cast<const pf4*>(wbase + (size_t)(kLstmH * g) * kLstmH + 4 * s);
#pragma unroll
            for (int et = 0; et < 4; ++et) {
              const pf4 hv = *reinterpret_cast<const pf4*>(hbase + (16 * et) * kLstmHLd + 4 * s);
              hb[et] = kp[et] ? hv : pf4{0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
              for (int et = 0; et < 4; ++et) acc[g][et] = pol_mfma4(wa[g], hb[et], acc[g][et]);
          }
        }
        // the cell in lstm_seq_fwd_kernel's arithmetic and order
#pragma unroll
        for (int et = 0; et < 4; ++et) {
          pf4 hn;
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const float ig = pol_sigm(acc[0][et][rr]);
            const float fg = pol_sigm(acc[1][et][rr]);
            const float gg = pol_tanh(acc[2][et][rr]);
            const float og = pol_sigm(acc[3][et][rr]);
            const float cp = kp[et] ? c[jb][et][rr] : 0.0f;
            const float cn = fg * cp + ig * gg;
            hn[rr] = og * pol_tanh(cn);
            c[jb][et][rr] = cn;
          }
          *reinterpret_cast<pf4*>(h_nxt + (16u * et + l16) * kLstmHLd + u0 + 4u * g4) = hn;
        }
      }
    }
    __syncthreads();   // B7: h'
    // ---- head: mean[row][a] = b[a] + sum_j h'[row][j] w[a][j], j ascending (policy_sample_kernel's dot) ----
    {
      const uint32_t row = t >> 2, ai = t & 3u;
      const pf4* hr = reinterpret_cast<const pf4*>(s_hp[nxt] + row * kLstmHLd);
      const pf4* wr = reinterpret_cast<const pf4*>(s_wh + ai * kLstmH);
      float dot = 0.0f;
      for (int j = 0; j < kLstmH / 4; ++j) {
        const pf4 hv = hr[j], wv = wr[j];
        dot = fmaf(hv.x, wv.x, dot);
        dot = fmaf(hv.y, wv.y, dot);
        dot = fmaf(hv.z, wv.z, dot);
        dot = fmaf(hv.w, wv.w, dot);
      }
      s_mean[t] = dot + p.b3[ai];
    }
    __syncthreads();   // B8
    if (wave != 0u) continue;

    // ---- the state wave: sample, then run_env's rollout step with the policy's action (quad_policy_rollout_kernel's
    // state wave, plus the next step's keep flag) ----
    const pf4 mv = *reinterpret_cast<const pf4*>(s_mean + 4u * lane);
    const float mean[OUZ_NUM_ACT] = {mv.x, mv.y, mv.z, mv.w};
    float eps[OUZ_NUM_ACT] = {0.0f, 0.0f, 0.0f, 0.0f};
    const size_t row_k = (size_t)k * n + (size_t)i;
    if (p.sample_mode == 0) {
      const U4 u = draw(p.sample_seed, gid, p.sample_call0 + (uint32_t)k, RNG_POLICY);
      eps[0] = normal_from(u.x, u.y, false);
      eps[1] = normal_from(u.x, u.y, true);
      eps[2] = normal_from(u.z, u.w, false);
      eps[3] = normal_from(u.z, u.w, true);
    } else if (p.sample_mode == 1 && valid) {
      const pf4 ev = *reinterpret_cast<const pf4*>(p.eps_in + row_k * OUZ_NUM_ACT);
      eps[0] = ev.x; eps[1] = ev.y; eps[2] = ev.z; eps[3] = ev.w;
    }
    float act[OUZ_NUM_ACT], logprob;
    pol_sample(mean, lsd, eps, act, logprob);
    if (valid) {
      *reinterpret_cast<pf4*>(p.action_out + row_k * OUZ_NUM_ACT) = pf4{act[0], act[1], act[2], act[3]};
      p.logprob_out[row_k] = logprob;
      if (p.eps_out) *reinterpret_cast<pf4*>(p.eps_out + row_k * OUZ_NUM_ACT) = pf4{eps[0], eps[1], eps[2], eps[3]};
    }
    S.act = make_float4(act[0], act[1], act[2], act[3]);

    float ob[OUZ_NUM_OBS];
#pragma unroll
    for (int j = 0; j < OUZ_NUM_OBS; ++j) ob[j] = 0.0f;
    float rew = 0.0f;
    bool rs = false, to = false;
    const bool did_reset = valid && S.rst;
    if (valid) env_core<CTRL, TGT, core_form(FORM)>(a, r.ctx[k], e, gid, TASK, S, ob, rew, rs, to);
    trace_count(a, r.ctx[k].step, did_reset, i, e);
    OutPtrs o = r.outs[0];   // rollout storage: row k of the (K, N, .) buffers; the env buffers get the last step
    o.obs += (size_t)k * n * OUZ_NUM_OBS;
    o.rew += (size_t)k * n;
    o.reset += (size_t)k * n;
    o.timeouts += (size_t)k * n;
    float* wave_lds = reinterpret_cast<float*>(s_obs4);
    emit(o, wave_lds, i, a.n, valid, ob, rew, rs, to, false);
    if (k == K - 1) emit(r.outs[1], wave_lds, i, a.n, valid, ob, rew, rs, to, false);

    // the learner-side corruption of the clean row, the next step's policy input and its keep flag
    float pom[OUZ_NUM_OBS];
    pol_corrupt(p, (uint32_t)i, k, ob, pom);
    if (valid && p.pomdp_out) pol_store_row(p.pomdp_out + row_k * OUZ_NUM_OBS, pom);
    float xin[OUZ_NUM_OBS];
#pragma unroll
    for (int j = 0; j < OUZ_NUM_OBS; ++j) xin[j] = p.acts_on_pomdp ? pom[j] : ob[j];
    pol_put_input(p, s_x, lane, valid, xin);
    s_keep[lane] = rs ? 0.0f : 1.0f;
  }

  // ---- the carry after the last step, its done not applied (s_hp[K & 1] was complete at the last step's B7) ----
  {
    const float* h_fin = s_hp[K & 1];
    for (uint32_t e4 = t; e4 < 64u * (kLstmH / 4); e4 += kPolBlock) {
      const uint32_t row = e4 / (kLstmH / 4), j4 = e4 % (kLstmH / 4);
      const size_t gi = tile0 + row;
      if (gi < n)
        *reinterpret_cast<pf4*>(q.h_out + gi * kLstmH + 4u * j4) =
            *reinterpret_cast<const pf4*>(h_fin + row * kLstmHLd + 4u * j4);
    }
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
      for (int et = 0; et < 4; ++et) {
        const size_t gi = tile0 + 16u * et + l16;
        if (gi < n) *reinterpret_cast<pf4*>(q.c_out + gi * kLstmH + 32u * wave + 16u * jb + 4u * g4) = c[jb][et];
      }
  }

  if (wave != 0u) return;   // (after the last barrier)
  if (sm && valid) {   // run_env's fused statistics
    const float s_tot = ep_sum_old + S.ep_sum_add;
    const int32_t c_tot = ep_cnt_old + S.ep_cnt_add, l_tot = ep_len_old + S.ep_len_add;
    ls.sum += (double)s_tot;
    ls.cnt += (double)c_tot;
    ls.len += (double)l_tot;
    if (sm == 2) {
      if (ep_cnt_old) {
        st(S.T, OUZ_F_EP_SUM, 0.0f);
        sti(S.T, OUZ_I_EP_CNT, 0);
        sti(S.T, OUZ_I_EP_LEN, 0);
      }
    } else if (S.ep_cnt_add) {
      st(S.T, OUZ_F_EP_SUM, s_tot);
      sti(S.T, OUZ_I_EP_CNT, c_tot);
      sti(S.T, OUZ_I_EP_LEN, l_tot);
    }
    S.ep_cnt_add = 0;
  }
  if (valid) env_store<CTRL, TGT, store_form(FORM)>(a, i, tp, S);
  if (sm) reduce_stats(r.stats, blockIdx.x, gridDim.x, ls);
}

}  // namespace ouz

static_assert(sizeof(ouz_policy_lstm) == 112, "ctypes OuzPolicyLstm mirror (ouzelum_amd/_lib.py)");
static_assert(sizeof(ouz_policy_lstm_carry) == 40, "ctypes OuzPolicyLstmCarry mirror");

extern "C" {

extern "C++" template <int T>
static void launch_lstm_policy_task(const StepArgs& a, const RolloutArgs& r, const PolicyArgs& p, const LstmArgs& q,
                                    dim3 g, hipStream_t s) {
  if constexpr (T == OUZ_TASK_OUZELUM || T == OUZ_TASK_FAULT || T == OUZ_TASK_LANDING) {
    hipLaunchKernelGGL((quad_lstm_policy_rollout_kernel<T>), g, dim3(kPolBlock), 0, s, a, r, p, q);
  }
}

int ouz_policy_rollout_lstm(ouz_env* env, const ouz_policy_lstm* lstm, const ouz_policy_lstm_carry* carry,
                            const ouz_policy_rollout_io* io, int32_t n_steps, double* stats_out, int32_t drain,
                            void* stream) {
  const char* fn = "ouz_policy_rollout_lstm";
  if (!env || !env->bound) return fail(OUZ_ERR_UNBOUND, std::string(fn) + ": env not bound");
  const int task = env->cfg.task;
  if (task != OUZ_TASK_OUZELUM && task != OUZ_TASK_FAULT && task != OUZ_TASK_LANDING)
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": the task must be Ouzelum, QuadFault or Landing");
  if (!lstm || !carry || !io) return fail(OUZ_ERR_INVALID, std::string(fn) + ": null lstm, carry or io");
  if (n_steps < 1) return fail(OUZ_ERR_INVALID, std::string(fn) + ": n_steps must be >= 1");
  if (!lstm->w1 || !lstm->b1 || !lstm->w2 || !lstm->b2 || !lstm->w_ih || !lstm->w_hh || !lstm->b_ih || !lstm->b_hh ||
      !lstm->w_head || !lstm->b_head || !lstm->logstd)
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": null weight tensor");
  if (!carry->h_in || !carry->c_in || !carry->done_in0 || !carry->h_out || !carry->c_out)
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": null carry tensor");
  if (carry->h_in == carry->h_out || carry->c_in == carry->c_out)
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": the carry's in and out tensors must be distinct");
  if ((lstm->norm_m == nullptr) != (lstm->norm_r == nullptr))
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": norm_m and norm_r: both or neither");
  if (lstm->norm_m && !(lstm->norm_clip > 0.0f)) return fail(OUZ_ERR_INVALID, std::string(fn) + ": norm_clip must be > 0");
  if (!io->act_in0 || !io->obs_out || !io->action_out || !io->logprob_out || !io->rew_out || !io->reset_out ||
      !io->timeouts_out)
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": null buffer");
  if (io->pomdp_mode < OUZ_POMDP_NONE || io->pomdp_mode > OUZ_POMDP_FLICKER_NOISE)
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": unknown pomdp_mode");
  if (io->pomdp_mode != OUZ_POMDP_NONE && !io->pomdp_out)
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": pomdp_out is null with a pomdp_mode other than NONE");
  if (io->sample_mode < 0 || io->sample_mode > 2) return fail(OUZ_ERR_INVALID, std::string(fn) + ": sample_mode is 0, 1 or 2");
  if (io->sample_mode == 1 && !io->eps_in) return fail(OUZ_ERR_INVALID, std::string(fn) + ": sample_mode 1 needs eps_in");
  const size_t n = (size_t)env->cfg.num_envs;
  if (io->pomdp_row_offset < 0 || io->pomdp_row_offset + (int64_t)n > 0xFFFFFFFFll)
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": bad pomdp_row_offset");
  // 16-byte accesses: the weights, the carry, the actions and the eps; the 13-wide rows as ouz_policy_rollout's
  const void* al[] = {lstm->w1, lstm->b1, lstm->w2, lstm->b2, lstm->w_ih, lstm->w_hh, lstm->b_ih, lstm->b_hh,
                      lstm->w_head, lstm->b_head, lstm->logstd, lstm->norm_m, lstm->norm_r, carry->h_in, carry->c_in,
                      carry->h_out, carry->c_out, io->action_out, io->eps_in, io->eps_out};
  for (const void* x : al)
    if (reinterpret_cast<uintptr_t>(x) & 15u) return fail(OUZ_ERR_INVALID, std::string(fn) + ": tensors must be 16-byte aligned");
  const void* al4[] = {io->act_in0, io->obs_out, io->pomdp_out, io->logprob_out, io->rew_out, carry->done_in0};
  for (const void* x : al4)
    if (reinterpret_cast<uintptr_t>(x) & 3u) return fail(OUZ_ERR_INVALID, std::string(fn) + ": f32 rows must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(io->reset_out) & 7u) return fail(OUZ_ERR_INVALID, std::string(fn) + ": reset_out must be 8-byte aligned");
  if (stats_out && !env->cfg.track_episodes)
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": stats_out needs an env created with track_episodes");
  const int stats_mode = stats_out ? (drain ? 2 : 1) : 0;
  const hipStream_t s = (hipStream_t)stream;
  const OutPtrs all_rows{io->obs_out, io->rew_out, io->reset_out, io->timeouts_out};
  const float* fed = (io->acts_on_pomdp && io->pomdp_out) ? io->pomdp_out : io->obs_out;   // the input of a later launch
  const float flick_p = io->pomdp_mode == OUZ_POMDP_FLICKER ? io->pomdp_prob : 0.1f;
  const bool flick = io->pomdp_mode == OUZ_POMDP_FLICKER || io->pomdp_mode == OUZ_POMDP_FLICKER_NOISE;
  for (int32_t k0 = 0; k0 < n_steps; k0 += kMaxRolloutChunk) {
    const int32_t K = (n_steps - k0) < kMaxRolloutChunk ? (n_steps - k0) : kMaxRolloutChunk;
    const OutPtrs rows = storage_row(all_rows, n, (size_t)k0);
    const size_t r0 = (size_t)k0 * n;
    RolloutArgs r;
    fill_rollout_args(env, r, K, &rows, io->action_out + r0 * OUZ_NUM_ACT, K, 0);
    if (stats_mode && k0 + K >= n_steps)
      r.stats = RolloutStats{stats_out, env->wave_partials, env->wave_ticket, stats_mode};
    PolicyArgs p{};
    p.w1 = lstm->w1; p.b1 = lstm->b1; p.w2 = lstm->w2; p.b2 = lstm->b2; p.w3 = lstm->w_head; p.b3 = lstm->b_head;
    p.logstd = lstm->logstd; p.norm_m = lstm->norm_m; p.norm_r = lstm->norm_r; p.norm_clip = lstm->norm_clip;
    p.acts_on_pomdp = io->acts_on_pomdp;
    p.in0 = k0 == 0 ? io->act_in0 : fed + (r0 - n) * OUZ_NUM_OBS;
    p.pomdp_out = io->pomdp_out ? io->pomdp_out + r0 * OUZ_NUM_OBS : nullptr;
    p.action_out = io->action_out + r0 * OUZ_NUM_ACT;
    p.logprob_out = io->logprob_out + r0;
    p.eps_in = io->eps_in ? io->eps_in + r0 * OUZ_NUM_ACT : nullptr;
    p.eps_out = io->eps_out ? io->eps_out + r0 * OUZ_NUM_ACT : nullptr;
    p.noise = io->pomdp_mode == OUZ_POMDP_NOISE || io->pomdp_mode == OUZ_POMDP_FLICKER_NOISE;
    p.noise_lo = (float)(1.0 - (double)io->pomdp_prob);   // ouz_pomdp_obs' range
    p.noise_hi = (float)(1.0 + (double)io->pomdp_prob);
    p.pomdp_seed = io->pomdp_seed;
    p.pomdp_row0 = (uint32_t)io->pomdp_row_offset;
    p.pomdp_call0 = io->pomdp_call0 + (uint32_t)k0;
    p.sample_mode = io->sample_mode;
    p.sample_seed = io->sample_seed;
    p.sample_call0 = io->sample_call0 + (uint32_t)k0;
    if (flick) {   // one coin per call for the whole batch, as ouz_pomdp_obs draws it
      for (int32_t k = 0; k < K; ++k)
        if (unit_f32(draw(io->pomdp_seed, BATCH_ENV, p.pomdp_call0 + (uint32_t)k, RNG_POMDP + SITE_LEARNER, 0u).x) <= flick_p)
          p.zero_mask |= 1u << k;
    }
    // a later chunk starts from the carry the chunk before left in h_out / c_out (in place: a workgroup reads its
    // rows first and writes them last) and from the stored reset row of the step before it
    LstmArgs q{};
    q.w_ih = lstm->w_ih; q.w_hh = lstm->w_hh; q.b_ih = lstm->b_ih; q.b_hh = lstm->b_hh;
    q.h_in = k0 == 0 ? carry->h_in : carry->h_out;
    q.c_in = k0 == 0 ? carry->c_in : carry->c_out;
    q.done_in0 = k0 == 0 ? carry->done_in0 : nullptr;
    q.reset_in0 = k0 == 0 ? nullptr : io->reset_out + (r0 - n);
    q.h_out = carry->h_out; q.c_out = carry->c_out;
    const dim3 g((unsigned)((n + 63) / 64));
    OUZ_TASK_SWITCH(task, launch_lstm_policy_task, (env->args, r, p, q, g, s))
    OUZ_LAUNCH_CHECK("quad_lstm_policy_rollout_kernel");
    env->step += K;
    prefill_flicker_masks(env, env->step, kMaxRolloutChunk);
  }
  return OUZ_OK;
}

}  // extern "C"
