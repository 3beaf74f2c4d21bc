// lrl_metrics.hip — evaluation metrics on the device (include/lrl.h LRL_METRIC_*): the per-step table and per-env
// totals of the reference's METRICS_FNS (mini_gym_learn/eval_metrics/metrics.py), and their reduction over an env group.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "lrl_kparams.h"
#include "lrl_launch.h"

namespace lrl {

// the table values follow torch's float32 op order (plain operators, unfused: see lrl_aux.hip)
#pragma clang fp contract(off)

// threads per env that share the height scan's rows (each a wave of 64 consecutive envs)
#define LRL_METRICS_HPARTS 16

// One thread per env, after the env kernel of the same lrl_sim_step: the step's post-physics state (no reset_idx has
// run yet) -> the per-step rows and the env's own column of the totals.  Coalesced: thread e reads row r of every
// SoA field at word e, as extras_snapshot_kernel does; lanes e >= n touch no memory.
// A workgroup is 64 consecutive envs x blockDim.y parts (wave-uniform part = threadIdx.y).  With a height scan its
// num_height_points rows are split over the parts (part p sums the points p, p + parts, ... in double; part 0 adds the
// partial sums in part order: a fixed order) -- one thread walking 187 rows is latency-bound; without a scan the launch
// has one part.  Everything else is part 0's.
__global__ __launch_bounds__(64 * LRL_METRICS_HPARTS) void metrics_kernel(const KParams* __restrict__ K, KState S,
                                                                          KMetrics M) {
  __shared__ double hsum[LRL_METRICS_HPARTS][64];
  const int lane = threadIdx.x, part = threadIdx.y, parts = blockDim.y;
  const int e = blockIdx.x * 64 + lane;
  const bool live = e < S.n;
  const int64_t N = S.stride;
  const lrl_env_params& P = K->p;
  const bool scan = P.measure_heights && P.num_height_points > 0;  // (uniform: every thread reaches the barrier)
  const float z = live ? S.root[2 * N + e] : 0.f;
  if (scan) {
    // root_z - measured_heights: the differences in float32 as the reference forms them, their sum in double
    double acc = 0.0;
    if (live)
      for (int k = part; k < P.num_height_points; k += parts) acc += (double)(z - S.heights[k * N + e]);
    hsum[part][lane] = acc;
    __syncthreads();
  }
  if (!live || part != 0) return;
  float v[LRL_METRIC_ROWS];
  const float vx = S.base_lin_vel[e], vy = S.base_lin_vel[N + e], wz = S.base_ang_vel[2 * N + e];
  const float dl = vx - S.commands[e], da = wz - S.commands[2 * N + e];
  v[LRL_METRIC_LIN_VEL_RMSD] = sqrtf(dl * dl);
  v[LRL_METRIC_ANG_VEL_RMSD] = sqrtf(da * da);
  v[LRL_METRIC_LIN_VEL_X] = vx;
  v[LRL_METRIC_ANG_VEL_YAW] = wz;
  if (scan) {
    double acc = 0.0;
    for (int p = 0; p < parts; ++p) acc += hsum[p][lane];
    v[LRL_METRIC_BASE_HEIGHT] = (float)(acc / (double)P.num_height_points);
  } else {
    v[LRL_METRIC_BASE_HEIGHT] = z;  // measured_heights is the scalar 0 there
  }
  float tmax = 0.f, power = 0.f;
  for (int k = 0; k < LRL_NUM_DOF; ++k) {
    const float tq = S.torques[k * N + e];
    tmax = fmaxf(tmax, fabsf(tq));
    power = power + tq * S.dof_vel[k * N + e];
  }
  v[LRL_METRIC_MAX_TORQUES] = tmax;
  v[LRL_METRIC_POWER_CONSUMPTION] = power;
  const float speed = sqrtf(vx * vx + vy * vy);
  const float mass = K->base_mass + S.payload[e];
  v[LRL_METRIC_COT] = power / ((mass * 9.8f) * speed);
  v[LRL_METRIC_FROUDE_NUMBER] = (vx * vx) / (float)(9.8 * 0.30);
  const int rst = S.reset[e] != 0, tout = S.time_out[e] != 0;
  v[LRL_METRIC_TERMINATION] = rst ? 1.f : 0.f;
  v[LRL_METRIC_SPEED_XY] = speed;
#pragma unroll
  for (int r = 0; r < LRL_METRIC_ROWS; ++r) {
    const int64_t i = r * N + e;
    M.step[i] = v[r];
    M.max[i] = fmaxf(M.max[i], v[r]);
    if (r == LRL_METRIC_COT) continue;  // never accumulated: inf / nan at zero speed
    const double d = (double)v[r];
    M.sum[i] += d;
    M.sumsq[i] += d * d;
  }
  M.steps[e] += 1;
  M.episodes[e] += rst;
  M.falls[e] += rst && !tout;
}

__global__ void metrics_clear_kernel(KState S, KMetrics M) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= S.n) return;
  const int64_t N = S.stride;
  for (int r = 0; r < LRL_METRIC_ROWS; ++r) {
    const int64_t i = r * N + e;
    M.sum[i] = 0.0;
    M.sumsq[i] = 0.0;
    M.max[i] = -INFINITY;
  }
  M.steps[e] = 0;
  M.episodes[e] = 0;
  M.falls[e] = 0;
}

// One workgroup pools the totals of the envs [first, first + count): thread t takes the envs first + t, first + t +
// 256, ... in that order, then an LDS tree per quantity — the same order every run.  out: LRL_METRICS_REDUCE_DOUBLES.
__global__ __launch_bounds__(256) void metrics_reduce_kernel(const KParams* __restrict__ K, KState S, KMetrics M,
                                                             int32_t first, int32_t count, double* __restrict__ out) {
  __shared__ double red[256];
  const int64_t N = S.stride;
  const int t = threadIdx.x;
  double sum[LRL_METRIC_ROWS], sq[LRL_METRIC_ROWS], mx[LRL_METRIC_ROWS], cnt[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r = 0; r < LRL_METRIC_ROWS; ++r) { sum[r] = 0.0; sq[r] = 0.0; mx[r] = -INFINITY; }
  for (int e = first + t; e < first + count && e < S.n; e += 256) {
    for (int r = 0; r < LRL_METRIC_ROWS; ++r) {
      const int64_t i = r * N + e;
      sum[r] += M.sum[i];
      sq[r] += M.sumsq[i];
      mx[r] = fmax(mx[r], (double)M.max[i]);
    }
    cnt[0] += (double)M.steps[e];
    cnt[1] += (double)M.episodes[e];
    cnt[2] += (double)M.falls[e];
    cnt[3] += (double)(K->base_mass + S.payload[e]) * M.sum[LRL_METRIC_SPEED_XY * N + e];
  }
  auto tree = [&](double x, bool is_max) {
    red[t] = x;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (t < s) red[t] = is_max ? fmax(red[t], red[t + s]) : red[t] + red[t + s];
      __syncthreads();
    }
    const double y = red[0];
    __syncthreads();
    return y;
  };
  for (int r = 0; r < LRL_METRIC_ROWS; ++r) {
    const double a = tree(sum[r], false), b = tree(sq[r], false), c = tree(mx[r], true);
    if (t == 0) { out[3 * r] = a; out[3 * r + 1] = b; out[3 * r + 2] = c; }
  }
  for (int k = 0; k < 4; ++k) {
    const double a = tree(cnt[k], false);
    if (t == 0) out[3 * LRL_METRIC_ROWS + k] = a;
  }
}

}  // namespace lrl

extern "C" {

hipError_t lrl_launch_metrics(const KParams* K, const KState* S, const KMetrics* M, int height_scan, hipStream_t st) {
  hipLaunchKernelGGL(lrl::metrics_kernel, dim3((S->n + 63) / 64), dim3(64, height_scan ? LRL_METRICS_HPARTS : 1), 0, st,
                     K, *S, *M);
  return hipGetLastError();
}

hipError_t lrl_launch_metrics_clear(const KState* S, const KMetrics* M, hipStream_t st) {
  hipLaunchKernelGGL(lrl::metrics_clear_kernel, dim3((S->n + 255) / 256), dim3(256), 0, st, *S, *M);
  return hipGetLastError();
}

hipError_t lrl_launch_metrics_reduce(const KParams* K, const KState* S, const KMetrics* M, int32_t first,
                                     int32_t count, double* out, hipStream_t st) {
  hipLaunchKernelGGL(lrl::metrics_reduce_kernel, dim3(1), dim3(256), 0, st, K, *S, *M, first, count, out);
  return hipGetLastError();
}

}  // extern "C"
