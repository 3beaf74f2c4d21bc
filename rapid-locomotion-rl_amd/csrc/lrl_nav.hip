// lrl_nav.hip — the navigation wrapper's step on the device (include/lrl.h lrl_nav_*; lrl/high_level.py restates the
// reference's scripts/high_level_play.py:131-249 in torch, and is the check for every line here).  One env per lane;
// the sim's fields are [field][stride], so a wave reads 64 consecutive floats of each, and the wrapper's own [n, k]
// buffers are small rows (k <= 14).  At 1,024 envs every kernel here is launch-bound: the step is split only where a
// value of every env is needed first (the "some env ends" test and the id list, then the means over the list).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lrl_kparams.h"
#include "lrl_launch.h"

namespace lrl {

// torch's float32 op order, uncontracted (the build is -ffp-contract=fast-honor-pragmas): norms are sqrtf of the
// squares summed left to right, a reward is value * float32(scale), sums add in list order.
#pragma clang fp contract(off)

constexpr int NB = LRL_NAV_BLOCK;
static_assert(NB % 64 == 0 && NB <= 1024, "whole waves");
static_assert(sizeof(lrl_nav_state) == LRL_NAV_STATE_BYTES, "lrl.h documents the size");

// base_pos = root[:, :3] - env_origins - base_init_state[:3], left to right
__device__ inline void nav_base_pos(const KState& S, const lrl_nav_state& V, int e, float p[3]) {
  const int64_t N = S.stride;
  for (int c = 0; c < 3; ++c) p[c] = (S.root[c * N + e] - S.env_origins[c * N + e]) - V.base_init_state[c];
}

// _reward_<term>() of env e from the wrapper's buffers as they stand (high_level_play.py:339-363): last_pos and
// last_actions are the previous step's until the last launch of the step, dist_travelled / lateral_vel / backward_vel /
// gs_buf / time_buf this step's once the first has run.
__device__ inline float nav_term(const KState& S, const lrl_nav_state& V, int e, int id) {
  switch (id) {
    case LRL_NAV_R_DISTANCE: {
      const float dx = V.last_pos[3 * e] - V.goal_position[2 * e];
      const float dy = V.last_pos[3 * e + 1] - V.goal_position[2 * e + 1];
      return sqrtf(dx * dx + dy * dy);
    }
    case LRL_NAV_R_ACTION_RATE: {
      float s = 0.f;
      for (int k = 0; k < 3; ++k) {
        const float d = V.last_actions[3 * e + k] - V.actions[3 * e + k];
        s = k == 0 ? d * d : s + d * d;
      }
      return s;
    }
    case LRL_NAV_R_LATERAL_VEL: return V.lateral_vel[e] * V.lateral_vel[e];
    case LRL_NAV_R_BACKWARD_VEL: return V.backward_vel[e] * V.backward_vel[e];
    case LRL_NAV_R_TERMINAL_DISTANCE_COVERED: return V.dist_travelled[e];
    case LRL_NAV_R_TERMINAL_DISTANCE_GS: return V.gs_buf[e] ? 1.f : 0.f;
    case LRL_NAV_R_TERMINAL_LL_RESET: return S.reset[e] ? 1.f : 0.f;
    case LRL_NAV_R_TERMINAL_TIME_OUT: return V.time_buf[e] ? 1.f : 0.f;
  }
  return 0.f;
}

// step() :127-131
__global__ __launch_bounds__(NB) void nav_begin_kernel(KState S, lrl_nav_state V, const float* __restrict__ actions) {
  const int e = blockIdx.x * NB + threadIdx.x;
  if (e >= V.n) return;
  float a[3];
  for (int k = 0; k < 3; ++k) {
    const float x = actions[3 * e + k];
    a[k] = x < -2.f ? -2.f : (x > 2.f ? 2.f : x);  // (a NaN stays a NaN, as torch.clamp)
  }
  const float keep = sqrtf(a[0] * a[0] + a[1] * a[1]) > V.command_threshold ? 1.f : 0.f;
  a[0] *= keep;  // a product: -0.0 for a zeroed negative command, as the reference's
  a[1] *= keep;
  for (int k = 0; k < 3; ++k) {
    V.actions[3 * e + k] = a[k];
    S.commands[(int64_t)k * S.stride + e] = a[k];
  }
}

// episode_length += 1, post_physics_step (:142-148), check_termination (:171-177) and compute_reward's step terms
// (:159-163).  Each workgroup also leaves the number of its envs whose reset flag is set.
__global__ __launch_bounds__(NB) void nav_flags_kernel(KState S, lrl_nav_state V) {
  __shared__ int wcnt[NB / 64];
  const int t = threadIdx.x, e = blockIdx.x * NB + t;
  bool rst = false;
  if (e < V.n) {
    const int64_t N = S.stride;
    const int ep = V.episode_length_buf[e] + 1;
    V.episode_length_buf[e] = ep;
    float p[3];
    nav_base_pos(S, V, e, p);
    const float d0 = p[0] - V.last_pos[3 * e], d1 = p[1] - V.last_pos[3 * e + 1], d2 = p[2] - V.last_pos[3 * e + 2];
    V.dist_travelled[e] += fabsf(sqrtf(d0 * d0 + d1 * d1 + d2 * d2));
    V.lateral_vel[e] = S.base_lin_vel[N + e];
    const float vx = S.base_lin_vel[e];
    V.backward_vel[e] = vx > 0.f ? 0.f : vx;  // clamp_max(v, 0)
    const float g0 = p[0] - V.goal_position[2 * e], g1 = p[1] - V.goal_position[2 * e + 1];
    const bool gs = sqrtf(g0 * g0 + g1 * g1) < V.goal_threshold;
    const bool tm = ep > V.max_episode_length;
    rst = V.reset_buf[e] != 0 || S.reset[e] != 0 || gs || tm;
    V.gs_buf[e] = gs;
    V.time_buf[e] = tm;
    V.reset_buf[e] = rst;
    float rew = 0.f;
    for (int i = 0; i < V.num_step_terms; ++i) {
      const float v = nav_term(S, V, e, V.term[i]) * V.scale[i];
      rew += v;
      V.episode_sums[(int64_t)i * V.n + e] += v;
    }
    V.rew_buf[e] = rew;
  }
  const unsigned long long m = __ballot(rst);
  if ((t & 63) == 0) wcnt[t >> 6] = __popcll(m);
  __syncthreads();
  if (t == 0) {
    int c = 0;
    for (int w = 0; w < NB / 64; ++w) c += wcnt[w];
    V.block_counts[blockIdx.x] = c;
  }
}

// compute_reward's terminal terms (:164-168: for every env, in steps where some env ends) and "total" (:169), and
// reset_buf.nonzero() (:177): every workgroup sums the workgroups' counts (the total, and those before it: its
// write offset), so the id list is ascending whatever order the workgroups run in.
__global__ __launch_bounds__(NB) void nav_reward_ids_kernel(KState S, lrl_nav_state V) {
  __shared__ int tot[NB], pre[NB], wcnt[NB / 64];
  const int t = threadIdx.x, e = blockIdx.x * NB + t;
  int a = 0, b = 0;
  for (int k = t; k < (int)gridDim.x; k += NB) {
    const int c = V.block_counts[k];
    a += c;
    if (k < (int)blockIdx.x) b += c;
  }
  tot[t] = a;
  pre[t] = b;
  __syncthreads();
  for (int w = NB / 2; w > 0; w >>= 1) {
    if (t < w) {
      tot[t] += tot[t + w];
      pre[t] += pre[t + w];
    }
    __syncthreads();
  }
  const int total = tot[0], first = pre[0];
  bool flag = false;
  if (e < V.n) {
    const int ns = V.num_step_terms, nt = V.num_terminal_terms;
    float rew = V.rew_buf[e];
    if (total > 0)
      for (int i = ns; i < ns + nt; ++i) {
        const float v = nav_term(S, V, e, V.term[i]) * V.scale[i];
        rew += v;
        V.episode_sums[(int64_t)i * V.n + e] += v;
      }
    V.episode_sums[(int64_t)(ns + nt) * V.n + e] += rew;
    V.rew_buf[e] = rew;
    flag = V.reset_buf[e] != 0;
  }
  const unsigned long long m = __ballot(flag);
  if ((t & 63) == 0) wcnt[t >> 6] = __popcll(m);
  __syncthreads();
  if (flag) {
    int o = first + __popcll(m & ((1ull << (t & 63)) - 1ull));
    for (int w = 0; w < (t >> 6); ++w) o += wcnt[w];
    if (o < V.n) V.ids[o] = e;  // (o < total <= n whenever the counts are this step's)
  }
  if (blockIdx.x == 0 && t == 0) V.count[0] = total;
}

// torch.mean(row[ids[lo:hi]]) in a fixed order: thread t takes lo + t, lo + t + 256, ..., then an LDS tree (the order
// of rows_mean_zero_kernel, lrl_aux.hip, which the host reset path runs).  Every thread returns the sum.
__device__ inline float nav_ids_sum(const float* row, const int32_t* ids, int lo, int hi, int n, float* red) {
  const int t = threadIdx.x;
  float s = 0.f;
  for (int i = lo + t; i < hi; i += 256) {
    const int id = ids[i];
    if ((unsigned)id < (unsigned)n) s += row[id];
  }
  red[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  const float y = red[0];
  __syncthreads();
  return y;
}

// reset_idx's logging (:182-195) of the wrapper's sum rows, one workgroup per row: the train group's mean, the eval
// group's first-finished-episode bookkeeping and mean, then the row's entries of the ids zeroed; the workgroups past
// the wrapper's rows do the low-level env's episode logging (legged_robot.py:261-276) on its own table.
__global__ __launch_bounds__(256) void nav_log_kernel(KState S, lrl_nav_state V, int32_t ll_rows) {
  __shared__ float red[256];
  __shared__ int ired[256];
  const int t = threadIdx.x, n = V.n;
  const int total = min(max(V.count[0], 0), n);
  const int R = V.num_step_terms + V.num_terminal_terms + 1;
  int r = blockIdx.x;
  if (r >= R) {
    r -= R;
    if (r >= ll_rows) return;
    if (total == 0) {
      if (V.prev_ll && t == 0) V.means_ll[r] = V.prev_ll[r];
      return;
    }
    float* row = S.episode_sums + (int64_t)r * S.stride;
    const float s = nav_ids_sum(row, V.ids, 0, total, n, red);
    if (t == 0) V.means_ll[r] = s / (float)total;
    for (int i = t; i < total; i += 256) {
      const int id = V.ids[i];
      if ((unsigned)id < (unsigned)n) row[id] = 0.f;
    }
    return;
  }
  int c = 0;  // the ids are ascending: the train envs' (id < num_train_envs) come first
  for (int i = t; i < total; i += 256) c += V.ids[i] < V.num_train_envs;
  ired[t] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) ired[t] += ired[t + w];
    __syncthreads();
  }
  const int ntr = ired[0];
  float* row = V.episode_sums + (int64_t)r * n;
  float* evr = V.episode_sums_eval + (int64_t)r * n;
  if (ntr > 0) {
    const float s = nav_ids_sum(row, V.ids, 0, ntr, n, red);
    if (t == 0) V.means_train[r] = s / (float)ntr;
  } else if (V.prev_train && t == 0) {
    V.means_train[r] = V.prev_train[r];
  }
  if (total > ntr) {
    for (int i = ntr + t; i < total; i += 256) {  // keep the first finished episode of each eval env
      const int id = V.ids[i];
      if ((unsigned)id < (unsigned)n && evr[id] == -1.f) evr[id] = row[id];
    }
    const float s = nav_ids_sum(row, V.ids, ntr, total, n, red);
    if (t == 0) V.means_eval[r] = s / (float)(total - ntr);
  } else if (V.prev_eval && t == 0) {
    V.means_eval[r] = V.prev_eval[r];
  }
  for (int i = t; i < total; i += 256) {  // (after nav_ids_sum's last barrier: every read of the row is done)
    const int id = V.ids[i];
    if ((unsigned)id < (unsigned)n) row[id] = 0.f;
  }
}

// The rest of reset_idx (:197-205) for the envs whose flag is still set — the batch the sim's reset kernel has just
// reset — with HistoryWrapper.reset_idx's zeroed history rows, then compute_observations (:150-156) and last_actions
// (:139) for every env.
__global__ __launch_bounds__(NB) void nav_finish_kernel(KState S, lrl_nav_state V, int32_t hist_floats) {
  __shared__ int list[NB];
  __shared__ int nlist;
  const int t = threadIdx.x, e = blockIdx.x * NB + t;
  if (t == 0) nlist = 0;
  __syncthreads();
  if (e < V.n) {
    const int64_t N = S.stride;
    if (V.reset_buf[e]) {
      V.rew_buf[e] = 0.f;
      V.episode_length_buf[e] = 0;
      V.lateral_vel[e] = 0.f;
      V.backward_vel[e] = 0.f;
      V.dist_travelled[e] = 0.f;
      V.reset_buf[e] = 0;
      list[atomicAdd(&nlist, 1)] = e;  // (an LDS integer counter: only the order of the zeroing below depends on it)
    }
    float p[3];
    nav_base_pos(S, V, e, p);
    float* o = V.obs_buf + (int64_t)e * 14;
    for (int c = 0; c < 3; ++c) {
      const float a = V.actions[3 * e + c];
      o[c] = p[c];
      o[3 + c] = S.base_lin_vel[c * N + e];
      o[6 + c] = S.base_ang_vel[c * N + e];
      o[9 + c] = a;
      V.last_pos[3 * e + c] = p[c];
      V.last_actions[3 * e + c] = a;
    }
    o[12] = V.goal_position[2 * e];
    o[13] = V.goal_position[2 * e + 1];
  }
  __syncthreads();
  const int k = nlist;
  for (int j = 0; j < k; ++j) {
    float* h = S.hist + (int64_t)list[j] * hist_floats;
    for (int i = t; i < hist_floats; i += NB) h[i] = 0.f;
  }
}

}  // namespace lrl

extern "C" {

hipError_t lrl_launch_nav_begin(const KState* S, const lrl_nav_state* V, const float* actions, hipStream_t st) {
  hipLaunchKernelGGL(lrl::nav_begin_kernel, dim3((V->n + lrl::NB - 1) / lrl::NB), dim3(lrl::NB), 0, st, *S, *V, actions);
  return hipGetLastError();
}

hipError_t lrl_launch_nav_flags(const KState* S, const lrl_nav_state* V, hipStream_t st) {
  const dim3 grid((V->n + lrl::NB - 1) / lrl::NB);
  hipLaunchKernelGGL(lrl::nav_flags_kernel, grid, dim3(lrl::NB), 0, st, *S, *V);
  hipLaunchKernelGGL(lrl::nav_reward_ids_kernel, grid, dim3(lrl::NB), 0, st, *S, *V);
  return hipGetLastError();
}

hipError_t lrl_launch_nav_log(const KState* S, const lrl_nav_state* V, int32_t ll_rows, hipStream_t st) {
  const int rows = V->num_step_terms + V->num_terminal_terms + 1 + ll_rows;
  hipLaunchKernelGGL(lrl::nav_log_kernel, dim3(rows), dim3(256), 0, st, *S, *V, ll_rows);
  return hipGetLastError();
}

hipError_t lrl_launch_nav_finish(const KState* S, const lrl_nav_state* V, int32_t hist_floats, hipStream_t st) {
  hipLaunchKernelGGL(lrl::nav_finish_kernel, dim3((V->n + lrl::NB - 1) / lrl::NB), dim3(lrl::NB), 0, st, *S, *V,
                     hist_floats);
  return hipGetLastError();
}

}  // extern "C"
