// lrl_env_dispatch.hip — the build-independent side of the env step: the dispatcher over the step kernel's three builds
// (lrl_env_layout.h; lrl_env_flat.hip, lrl_env_mesh.hip and lrl_env_mesh_tgs.hip hold one each) and observe_kernel, the
// re-evaluation of the observations of envs reset inside a step, built on the step kernel's helpers (lrl_env_step.h).
#include "lrl_env_step.h"

// mesh_tgs: the sim's parameters ask for TGS on the mesh (terrain_mesh, solver_tgs, solver_iterations > 0)
extern "C" hipError_t lrl_launch_env_step(const KParams* K, const KState* S, int lds_bytes, const float* actions,
                                          uint32_t flags, int64_t step_counter, int terrain_mesh, int mesh_tgs,
                                          hipStream_t stream) {
  if (!terrain_mesh) return lrl_launch_env_step_plane(K, S, lds_bytes, actions, flags, step_counter, stream);
  if (mesh_tgs) return lrl_launch_env_step_mesh_tgs(K, S, lds_bytes, actions, flags, step_counter, stream);
  return lrl_launch_env_step_mesh(K, S, lds_bytes, actions, flags, step_counter, stream);
}

// the three builds' setup / debug entry points, for the loops below
#define LRL_X(b) {lrl_env_kernel_setup_##b, lrl_debug_env_profile_##b, lrl_debug_env_buffer_##b},
static const struct {
  hipError_t (*setup)(int);
  int (*profile)(unsigned long long*, int);
  int (*buffer)(float*);
} kBuilds[] = {LRL_ENV_BUILDS(LRL_X)};
#undef LRL_X

extern "C" hipError_t lrl_env_kernel_setup(int lds_bytes) {
  hipError_t e = hipSuccess;
  for (const auto& b : kBuilds)
    if (e == hipSuccess) e = b.setup(lds_bytes);
  return e;
}
// the sum of the three builds' timers (a simulation runs one of them); 0: not a profile build
extern "C" int lrl_debug_env_profile(unsigned long long* out, int reset) {
  unsigned long long sum[24] = {0}, t[24];
  for (const auto& b : kBuilds) {
    const int n = b.profile(t, reset);
    if (n != 24) return n ? -2 : 0;
    for (int i = 0; i < 24; ++i) sum[i] += t[i];
  }
  for (int i = 0; i < 24; ++i) out[i] = sum[i];
  return 24;
}
// 0: not a debug build
extern "C" int lrl_debug_env_buffer(float* buf) {
  for (const auto& b : kBuilds)
    if (const int r = b.buffer(buf); r != 1) return r ? -2 : 0;
  return 1;
}

#pragma clang fp contract(off)  // (as the helpers: torch's op order)
namespace lrl {
// compute_observations for envs just reset inside a step (upstream semantics, legged_robot.py:177-184):
// obs / priv rows from the post-reset state with the step's noise draws, the newest history slot, and the
// last_* buffers post_physics_step sets after the reset (last_actions = actions, last_dof_vel = dof_vel,
// last_root_vel = root velocity).  One thread per listed env.
// 16 lanes per env (OBS_LANES): lane c forms, noises, clips and stores only its 4-wide chunks of the observation row
// (chunk i0 / 4 on lane (i0 / 4) % 16: one Philox draw each instead of the whole row's draws on one thread), reading
// the state entries those need; lane 0 writes the base-frame velocities, the privileged row and the last_* buffers.
// Every element's value, draw and operation order are the step kernel's (obs_base_values + its quads' joint entries /
// obs_noise_clip), so the rows are bit-identical.
constexpr int OBS_LANES = 16;
// observation entry i of env e (the step kernel's layout: [only lin vel,] [only ang vel,] [lin vel, ang vel,] gravity,
// [commands,] dof pos, dof vel, actions, [yaw,] then the height rows against base height z)
__device__ __forceinline__ float obs_entry(const lrl_env_params& P, const KState& S, int e, int i, V3 blv, V3 bav,
                                           V3 pg) {
  const int N = S.stride;
  int o = 0;
  if (P.observe_only_lin_vel) {
    if (i < 3) return (i == 0 ? blv.x : i == 1 ? blv.y : blv.z) * P.obs_scale_lin_vel;
    o = 3;
  }
  if (P.observe_only_ang_vel) {
    if (i < o + 3) return (i == o ? bav.x : i == o + 1 ? bav.y : bav.z) * P.obs_scale_ang_vel;
    o += 3;
  }
  if (P.observe_vel) {
    if (i < o + 3)
      return (P.global_reference ? S.root[(7 + i - o) * N + e] : (i == o ? blv.x : i == o + 1 ? blv.y : blv.z)) *
             P.obs_scale_lin_vel;
    if (i < o + 6) return (i == o + 3 ? bav.x : i == o + 4 ? bav.y : bav.z) * P.obs_scale_ang_vel;
    o += 6;
  }
  if (i < o + 3) return i == o ? pg.x : i == o + 1 ? pg.y : pg.z;
  o += 3;
  if (P.observe_command) {
    if (i < o + 3) return S.commands[(i - o) * N + e] * P.commands_scale[i - o];
    o += 3;
  }
  if (i < o + 12) return (S.dof_pos[(i - o) * N + e] - P.default_dof_pos[i - o]) * P.obs_scale_dof_pos;
  if (i < o + 24) return S.dof_vel[(i - o - 12) * N + e] * P.obs_scale_dof_vel;
  if (i < o + 36) return S.actions[(i - o - 24) * N + e];
  if (P.observe_yaw && i == o + 36) {
    float q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = S.root[(3 + k) * N + e];
    return obs_yaw_value(q);
  }
  const int k = i - (P.num_obs - P.num_height_points);  // height row k (measure_heights)
  return fminf(fmaxf(S.root[2 * N + e] - 0.5f - S.heights[k * N + e], -1.f), 1.f) * P.obs_scale_height;
}
__global__ __launch_bounds__(256) void observe_kernel(const KParams* __restrict__ K, KState S,
                                                      const int32_t* __restrict__ ids, int32_t n,
                                                      const int32_t* __restrict__ dn, uint32_t flags,
                                                      int64_t step_counter) {
  const int gt = blockIdx.x * blockDim.x + threadIdx.x;
  const int t = gt / OBS_LANES, c = gt % OBS_LANES;
  if (t >= (dn ? min(*dn, n) : n)) return;  // (dn: device count, n its bound)
  const int e = ids[t];
  if (e < 0 || e >= S.n) return;
  const lrl_env_params& P = K->p;
  const int N = S.stride, NO = P.num_obs;
  const uint64_t genv = (uint64_t)(S.env_offset + e);
  const bool inject = (flags & LRL_STEP_INJECT_UNIFORM) != 0;
  float quat[4], V[3], W[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) quat[k] = S.root[(3 + k) * N + e];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    V[k] = S.root[(7 + k) * N + e];
    W[k] = S.root[(10 + k) * N + e];
  }
  const V3 blv = quat_rotate_inverse(quat, v3(V[0], V[1], V[2]));
  const V3 bav = quat_rotate_inverse(quat, v3(W[0], W[1], W[2]));
  const V3 pg = quat_rotate_inverse(quat, v3(0.f, 0.f, -1.f));
  float* row = S.obs + (size_t)e * NO;
  float* h = (flags & LRL_STEP_HISTORY) ? S.hist + (size_t)e * (K->num_history * NO) + (K->num_history - 1) * NO
                                        : nullptr;
  for (int i0 = 4 * c; i0 < NO; i0 += 4 * OBS_LANES) {
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = i0 + k < NO ? obs_entry(P, S, e, i0 + k, blv, bav, pg) : 0.f;
    if (P.add_noise) {  // (obs_noise_clip's chunk i0 / 4)
      lrl_u32x4 r = lrl_philox((uint32_t)genv, (uint32_t)step_counter,
                               (LRL_RNG_OBS_NOISE << 16) ^ (uint32_t)(step_counter >> 32), (uint32_t)(i0 >> 2), S.seed);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k;
        if (i < NO) {
          float u = inject ? (e < S.n ? S.inj_noise[(size_t)e * NO + i] : 0.5f) : lrl_u01(r.v[k]);
          v[k] += (2.f * u - 1.f) * P.noise_vec[i];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k < NO) {
        const float x = fminf(fmaxf(v[k], -P.clip_obs), P.clip_obs);
        row[i0 + k] = x;
        if (h) h[i0 + k] = x;
      }
  }
  if (c != 0) return;
  float ms[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) ms[j] = S.motor_strength[j * N + e];
  S.base_lin_vel[e] = blv.x; S.base_lin_vel[N + e] = blv.y; S.base_lin_vel[2 * N + e] = blv.z;
  S.base_ang_vel[e] = bav.x; S.base_ang_vel[N + e] = bav.y; S.base_ang_vel[2 * N + e] = bav.z;
  S.projected_gravity[e] = pg.x; S.projected_gravity[N + e] = pg.y; S.projected_gravity[2 * N + e] = pg.z;
  priv_row(P, S, e, S.payload[e], v3(S.com[e], S.com[N + e], S.com[2 * N + e]), ms, S.priv + (size_t)e * LRL_NUM_PRIV);
#pragma unroll
  for (int j = 0; j < 12; ++j) {
    S.last_actions[j * N + e] = S.actions[j * N + e];
    S.last_dof_vel[j * N + e] = S.dof_vel[j * N + e];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    S.last_root_vel[k * N + e] = V[k];
    S.last_root_vel[(3 + k) * N + e] = W[k];
  }
}
}  // namespace lrl

extern "C" hipError_t lrl_launch_observe(const KParams* K, const KState* S, const int32_t* ids, int32_t n,
                                         const int32_t* dn, uint32_t flags, int64_t step_counter, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(lrl::observe_kernel, dim3((int)(((int64_t)n * lrl::OBS_LANES + 255) / 256)), dim3(256), 0, stream,
                     K, *S, ids, n, dn, flags, step_counter);
  return hipGetLastError();
}
