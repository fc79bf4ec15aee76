// ouz_policy_rollout: the fused rollout with the 13 -> 256 -> 256 -> 4 tanh MLP actor in the loop.
// Included at the end of quad_kernels.hip: the env side is run_env's rollout loop (env_load once, K x (env_core +
// outputs), env_store once) in the general form, with the next step's action taken from the policy in place of
// load_actions.
//
// One workgroup of four waves per 64-env tile.  A policy's action for env i at step k depends on env i's observation
// only, so a tile carries its own policy evaluation through the K steps of a launch and the waves meet at
// __syncthreads() alone: five barriers per step, reached by every wave of every workgroup K times (K is a kernel
// argument; a partial tile's idle lanes hold zero input rows and store nothing).
//   step k:  [B1] layer 1 (all 256 threads: thread t owns hidden unit t, the tile's 64 input rows from LDS)
//            [B2] layer 2 on v_mfma_f32_16x16x4_f32 (wave w owns units 64 w .. 64 w + 63 of all 64 rows)
//            [B3] bias + tanh of the accumulators back into the activation buffer, in place
//            [B4] head: thread t = 4 row + a, one dot product of 256
//            [B5] wave 0, the state wave: sample, log-prob, stores, env step, outputs, the learner-side corruption,
//                 the next policy input into LDS; waves 1-3 wait at the next step's B1.
// Every output element is a sum over k in one fixed order that does not depend on the row's place in the tile or on
// the shard: a sharded run reproduces the unsharded one bit for bit.
#pragma once

namespace ouz {

constexpr int kPolH = 256;            // hidden width (PPO/model.py:11-40)
constexpr int kPolLd = kPolH + 4;     // activation row stride in LDS, floats (16-byte aligned rows, banks 4 apart)
constexpr int kPolXLd = 16;           // input row stride: 13 values + 3 zeros, four 16-byte reads
constexpr int kPolBlock = 256;
typedef float pf4 __attribute__((ext_vector_type(4)));

struct PolicyArgs {
  const float *w1, *b1, *w2, *b2, *w3, *b3, *logstd, *norm_m, *norm_r;
  float norm_clip;
  int32_t acts_on_pomdp;
  // rows of this launch's first step ([K][N][.] buffers) and the [N][13] input of its first step
  const float* in0;
  float* pomdp_out;
  float* action_out;
  float* logprob_out;
  const float* eps_in;
  float* eps_out;
  uint32_t zero_mask;       // bit k: the whole-batch flicker coin of step k zeroes the batch (host-drawn)
  int32_t noise;
  float noise_lo, noise_hi;
  uint64_t pomdp_seed;
  uint32_t pomdp_row0, pomdp_call0;
  int32_t sample_mode;
  uint32_t sample_call0;
  uint64_t sample_seed;
};

// learner_kernels.hip's ftanh (hardware exp2 / rcp, ~1e-7 absolute) and norm_forward, restated for this unit
__device__ __forceinline__ float pol_tanh(float x) {
  const float t = __builtin_amdgcn_exp2f(-2.88539008177792681f * fabsf(x));
  return copysignf((1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t), x);
}
__device__ __forceinline__ float pol_norm(float x, float m, float r, float clip) {
#pragma clang fp contract(off)
  float y = (x - m) * r;
  y = y < -clip ? -clip : y;
  y = y > clip ? clip : y;
  return y;
}

// pomdp_obs_kernel's row (learner_kernels.hip): key (seed, row0 + row, call, RNG_POMDP + SITE_LEARNER, 128 + g)
__device__ __forceinline__ void pol_corrupt(const PolicyArgs& p, uint32_t row, int k, const float* x, float* y) {
#pragma clang fp contract(off)
  const bool zero = (p.zero_mask >> k) & 1u;
#pragma unroll
  for (int g = 0; g < (OUZ_NUM_OBS + 3) / 4; ++g) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (p.noise) {
      const U4 u = draw(p.pomdp_seed, p.pomdp_row0 + row, p.pomdp_call0 + (uint32_t)k, RNG_POMDP + SITE_LEARNER,
                        128u + (uint32_t)g);
      w[0] = u.x; w[1] = u.y; w[2] = u.z; w[3] = u.w;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = g * 4 + j;
      if (e < OUZ_NUM_OBS) {
        float v = zero ? 0.0f : x[e];
        if (p.noise) v = v * uniform_f32(w[j], p.noise_lo, p.noise_hi);
        y[e] = v;
      }
    }
  }
}

// policy_sample_kernel's arithmetic for one row held by one lane: action = mean + exp(logstd) eps and
// log-prob = -(sum logstd + 4 log sqrt(2 pi)) - 1/2 sum eps^2, the sums in its shuffle order (0 + 1) + (2 + 3)
__device__ __forceinline__ void pol_sample(const float* mean, const float* ls, const float* e, float* act, float& logprob) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < OUZ_NUM_ACT; ++j) act[j] = mean[j] + expf(ls[j]) * e[j];
  const float q = (e[0] * e[0] + e[1] * e[1]) + (e[2] * e[2] + e[3] * e[3]);
  const float lsum = (ls[0] + ls[1]) + (ls[2] + ls[3]);
  const float kLogSqrt2Pi = 0.918938533204672742f;
  const float c = lsum + (float)OUZ_NUM_ACT * kLogSqrt2Pi;
  logprob = -c + (-0.5f) * q;
}

// One 13-float row at r (4-byte aligned): three 16-byte stores + one dword, as emit's latency-regime form
__device__ __forceinline__ void pol_store_row(float* r, const float* v) {
  typedef float f4a4 __attribute__((ext_vector_type(4), aligned(4)));
  *reinterpret_cast<f4a4*>(r) = f4a4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f4a4*>(r + 4) = f4a4{v[4], v[5], v[6], v[7]};
  *reinterpret_cast<f4a4*>(r + 8) = f4a4{v[8], v[9], v[10], v[11]};
  r[12] = v[12];
}

// The policy's input row of one lane into LDS: normalised when the constants are given; an idle lane's row is zero
__device__ __forceinline__ void pol_put_input(const PolicyArgs& p, float* s_x, uint32_t lane, bool valid, const float* x) {
  const bool norm = p.norm_m != nullptr;
#pragma unroll
  for (int j = 0; j < OUZ_NUM_OBS; ++j) {
    float v = x[j];
    if (norm) v = pol_norm(v, p.norm_m[j], p.norm_r[j], p.norm_clip);
    s_x[lane * kPolXLd + j] = valid ? v : 0.0f;
  }
}

template <int TASK>
__global__ void __launch_bounds__(kPolBlock) quad_policy_rollout_kernel(StepArgs a, RolloutArgs r, PolicyArgs p) {
  constexpr int CTRL = task_ctrl(TASK), TGT = task_tgt(TASK);
  constexpr unsigned FORM = F_MULTI;   // the general one-wave rollout form: DR, trace and lazy resets as configured
  static_assert(CTRL == CTRL_RL, "the tasks whose step takes the policy's action");
  __shared__ float s_h[64 * kPolLd];            // activations of the tile: layer 1's, then layer 2's in place
  __shared__ float s_x[64 * kPolXLd];           // policy input rows
  __shared__ float s_w3[OUZ_NUM_ACT * kPolH];   // the head's weights
  __shared__ float s_mean[64 * OUZ_NUM_ACT];
  __shared__ float4 s_obs4[64 * OUZ_NUM_OBS / 4];   // emit's staging (the state wave's)
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, l16 = lane & 15u, g4 = lane >> 4;
  const int K = r.K;
  const size_t n = (size_t)a.n;

  // ---- launch prologue: weights that stay on chip, the state, the first input ----
  *reinterpret_cast<pf4*>(s_w3 + 4 * t) = *reinterpret_cast<const pf4*>(p.w3 + 4 * t);
  float w1r[OUZ_NUM_OBS];
#pragma unroll
  for (int j = 0; j < OUZ_NUM_OBS; ++j) w1r[j] = p.w1[t * OUZ_NUM_OBS + j];
  const float b1t = p.b1[t];
  for (uint32_t j = t; j < 64u * kPolXLd; j += kPolBlock) s_x[j] = 0.0f;   // (the three pad columns stay zero)
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
    __syncthreads();   // B1: the input rows of step k
    // ---- layer 1: h1[row][t] = tanh(b1[t] + sum_j x[row][j] w1[t][j]), j ascending ----
    for (int row = 0; row < 64; ++row) {
      const pf4* xr = reinterpret_cast<const pf4*>(s_x + row * kPolXLd);
      const pf4 x0 = xr[0], x1 = xr[1], x2 = xr[2], x3 = xr[3];
      float acc = b1t;
      acc = fmaf(x0.x, w1r[0], acc); acc = fmaf(x0.y, w1r[1], acc); acc = fmaf(x0.z, w1r[2], acc); acc = fmaf(x0.w, w1r[3], acc);
      acc = fmaf(x1.x, w1r[4], acc); acc = fmaf(x1.y, w1r[5], acc); acc = fmaf(x1.z, w1r[6], acc); acc = fmaf(x1.w, w1r[7], acc);
      acc = fmaf(x2.x, w1r[8], acc); acc = fmaf(x2.y, w1r[9], acc); acc = fmaf(x2.z, w1r[10], acc); acc = fmaf(x2.w, w1r[11], acc);
      acc = fmaf(x3.x, w1r[12], acc);
      s_h[row * kPolLd + t] = pol_tanh(acc);
    }
    __syncthreads();   // B2
    // ---- layer 2, transposed as the LSTM sequence kernels do: out^T = W2 h1^T.  The weight tile is the MFMA's A
    // operand (unit l & 15 of the tile), the activation tile its B operand (row l & 15), so lane l holds units
    // 4 (l >> 4) + 0..3 of row l & 15: one 16-byte LDS store per tile.  k order: lane group l >> 4 walks
    // k = 64 (l >> 4) + 4 s .. + 3, so four consecutive MFMA steps take one 16-byte load per operand. ----
    pf4 acc[4][4];
#pragma unroll
    for (int ut = 0; ut < 4; ++ut)
#pragma unroll
      for (int et = 0; et < 4; ++et) acc[ut][et] = pf4{0.0f, 0.0f, 0.0f, 0.0f};
    const float* wbase = p.w2 + (size_t)(64u * wave + l16) * kPolH + 64u * g4;
    const float* hbase = s_h + l16 * kPolLd + 64u * g4;
#pragma unroll 2
    for (int s = 0; s < 16; ++s) {
      pf4 wa[4], hb[4];
#pragma unroll
      for (int ut = 0; ut < 4; ++ut) wa[ut] = *reinterpret_cast<const pf4*>(wbase + (size_t)(16 * ut) * kPolH + 4 * s);
#pragma unroll
      for (int et = 0; et < 4; ++et) hb[et] = *reinterpret_cast<const pf4*>(hbase + (16 * et) * kPolLd + 4 * s);
#pragma unroll
      for (int ut = 0; ut < 4; ++ut)
#pragma unroll
        for (int et = 0; et < 4; ++et) {
          pf4 c = acc[ut][et];
          c = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[ut].x, hb[et].x, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[ut].y, hb[et].y, c, 0, 0, 0);
          c = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[ut].z, hb[et].z, c, 0, 0, 0);
          acc[ut][et] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[ut].w, hb[et].w, c, 0, 0, 0);
        }
    }
    __syncthreads();   // B3: every wave has read h1
#pragma unroll
    for (int ut = 0; ut < 4; ++ut) {
      const uint32_t unit0 = 64u * wave + 16u * ut + 4u * g4;
      const pf4 b2v = *reinterpret_cast<const pf4*>(p.b2 + unit0);
#pragma unroll
      for (int et = 0; et < 4; ++et) {
        const pf4 v = acc[ut][et] + b2v;
        *reinterpret_cast<pf4*>(s_h + (16u * et + l16) * kPolLd + unit0) =
            pf4{pol_tanh(v.x), pol_tanh(v.y), pol_tanh(v.z), pol_tanh(v.w)};
      }
    }
    __syncthreads();   // B4
    // ---- head: mean[row][a] = b3[a] + sum_j h2[row][j] w3[a][j], j ascending (policy_sample_kernel's dot) ----
    {
      const uint32_t row = t >> 2, ai = t & 3u;
      const pf4* hr = reinterpret_cast<const pf4*>(s_h + row * kPolLd);
      const pf4* wr = reinterpret_cast<const pf4*>(s_w3 + ai * kPolH);
      float dot = 0.0f;
      for (int j = 0; j < kPolH / 4; ++j) {
        const pf4 hv = hr[j], wv = wr[j];
        dot = fmaf(hv.x, wv.x, dot);
        dot = fmaf(hv.y, wv.y, dot);
        dot = fmaf(hv.z, wv.z, dot);
        dot = fmaf(hv.w, wv.w, dot);
      }
      s_mean[t] = dot + p.b3[ai];
    }
    __syncthreads();   // B5
    if (wave != 0u) continue;

    // ---- the state wave: sample, then run_env's rollout step with the policy's action ----
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

    // the learner-side corruption of the clean row, and the next step's policy input
    float pom[OUZ_NUM_OBS];
    pol_corrupt(p, (uint32_t)i, k, ob, pom);
    if (valid && p.pomdp_out) pol_store_row(p.pomdp_out + row_k * OUZ_NUM_OBS, pom);
    float xin[OUZ_NUM_OBS];
#pragma unroll
    for (int j = 0; j < OUZ_NUM_OBS; ++j) xin[j] = p.acts_on_pomdp ? pom[j] : ob[j];
    pol_put_input(p, s_x, lane, valid, xin);
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

static_assert(sizeof(ouz_policy_mlp) == 80, "ctypes OuzPolicyMlp mirror (ouzelum_amd/_lib.py)");
static_assert(sizeof(ouz_policy_rollout_io) == 136, "ctypes OuzPolicyRolloutIo mirror");

extern "C" {

extern "C++" template <int T>
static void launch_policy_task(const StepArgs& a, const RolloutArgs& r, const PolicyArgs& p, dim3 g, hipStream_t s) {
  if constexpr (T == OUZ_TASK_OUZELUM || T == OUZ_TASK_FAULT || T == OUZ_TASK_LANDING) {
    hipLaunchKernelGGL((quad_policy_rollout_kernel<T>), g, dim3(kPolBlock), 0, s, a, r, p);
  }
}

int ouz_policy_rollout(ouz_env* env, const ouz_policy_mlp* mlp, const ouz_policy_rollout_io* io, int32_t n_steps,
                       double* stats_out, int32_t drain, void* stream) {
  const char* fn = "ouz_policy_rollout";
  if (!env || !env->bound) return fail(OUZ_ERR_UNBOUND, std::string(fn) + ": env not bound");
  const int task = env->cfg.task;
  if (task != OUZ_TASK_OUZELUM && task != OUZ_TASK_FAULT && task != OUZ_TASK_LANDING)
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": the task must be Ouzelum, QuadFault or Landing");
  if (!mlp || !io) return fail(OUZ_ERR_INVALID, std::string(fn) + ": null mlp or io");
  if (n_steps < 1) return fail(OUZ_ERR_INVALID, std::string(fn) + ": n_steps must be >= 1");
  if (!mlp->w1 || !mlp->b1 || !mlp->w2 || !mlp->b2 || !mlp->w3 || !mlp->b3 || !mlp->logstd)
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": null weight tensor");
  if ((mlp->norm_m == nullptr) != (mlp->norm_r == nullptr))
    return fail(OUZ_ERR_INVALID, std::string(fn) + ": norm_m and norm_r: both or neither");
  if (mlp->norm_m && !(mlp->norm_clip > 0.0f)) return fail(OUZ_ERR_INVALID, std::string(fn) + ": norm_clip must be > 0");
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
  // 16-byte accesses: the weights, the actions and the eps.  The 13-wide rows (act_in0, obs_out, pomdp_out) are read
  // and written with 4-byte alignment, as ouz_rollout's storage rows are, so they may be rows of a larger tensor.
  const void* al[] = {mlp->w1, mlp->b1, mlp->w2, mlp->b2, mlp->w3, mlp->b3, mlp->logstd, mlp->norm_m, mlp->norm_r,
                      io->action_out, io->eps_in, io->eps_out};
  for (const void* q : al)
    if (reinterpret_cast<uintptr_t>(q) & 15u) return fail(OUZ_ERR_INVALID, std::string(fn) + ": tensors must be 16-byte aligned");
  const void* al4[] = {io->act_in0, io->obs_out, io->pomdp_out, io->logprob_out, io->rew_out};
  for (const void* q : al4)
    if (reinterpret_cast<uintptr_t>(q) & 3u) return fail(OUZ_ERR_INVALID, std::string(fn) + ": f32 rows must be 4-byte aligned");
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
    // (ctx[k].actions: row k of action_out, valid memory for env_load's action load; the step takes the policy's)
    fill_rollout_args(env, r, K, &rows, io->action_out + r0 * OUZ_NUM_ACT, K, 0);
    if (stats_mode && k0 + K >= n_steps)
      r.stats = RolloutStats{stats_out, env->wave_partials, env->wave_ticket, stats_mode};
    PolicyArgs p{};
    p.w1 = mlp->w1; p.b1 = mlp->b1; p.w2 = mlp->w2; p.b2 = mlp->b2; p.w3 = mlp->w3; p.b3 = mlp->b3;
    p.logstd = mlp->logstd; p.norm_m = mlp->norm_m; p.norm_r = mlp->norm_r; p.norm_clip = mlp->norm_clip;
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
    const dim3 g((unsigned)((n + 63) / 64));
    OUZ_TASK_SWITCH(task, launch_policy_task, (env->args, r, p, g, s))
    OUZ_LAUNCH_CHECK("quad_policy_rollout_kernel");
    env->step += K;
    prefill_flicker_masks(env, env->step, kMaxRolloutChunk);
  }
  return OUZ_OK;
}

}  // extern "C"
