// Internal extern "C" functions that cross translation units inside liblrl.so: the kernel launchers lrl_capi.cpp calls
// and the error setter the other files call back.  Every file that defines one includes this header, so the compiler
// compares the definition with the declaration its callers see (extern "C" names carry no argument types).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lrl_env_layout.h"

extern "C" {
int lrl_set_error(int code, const char* msg);  // lrl_capi.cpp: sets the thread's lrl_last_error, returns code
// lrl_env_dispatch.hip (mesh_tgs: the sim's parameters ask for TGS on the mesh)
hipError_t lrl_launch_env_step(const KParams* K, const KState* S, int lds_bytes, const float* actions, uint32_t flags,
                               int64_t step_counter, int terrain_mesh, int mesh_tgs, hipStream_t stream);
hipError_t lrl_launch_observe(const KParams*, const KState*, const int32_t*, int32_t, const int32_t*, uint32_t, int64_t,
                              hipStream_t);
hipError_t lrl_env_kernel_setup(int lds_bytes);
int lrl_debug_env_profile(unsigned long long* out, int reset);
int lrl_debug_env_buffer(float* buf);
// one build of the env step kernel (lrl_env_flat.hip, lrl_env_mesh.hip, lrl_env_mesh_tgs.hip: LRL_ENV_ENTRY_POINTS)
#define LRL_ENV_ENTRY_DECLS(b)                                                                              \
  hipError_t lrl_launch_env_step_##b(const KParams*, const KState*, int, const float*, uint32_t, int64_t, hipStream_t); \
  hipError_t lrl_env_kernel_setup_##b(int lds_bytes);                                                       \
  int lrl_debug_env_profile_##b(unsigned long long* out, int reset);                                        \
  int lrl_debug_env_buffer_##b(float* buf);
LRL_ENV_BUILDS(LRL_ENV_ENTRY_DECLS)
// lrl_aux.hip
hipError_t lrl_launch_reset(const KParams*, const KState*, const int32_t*, int32_t, const int32_t*, int32_t, float, float,
                            float, float, int32_t, hipStream_t);
hipError_t lrl_launch_env_lists(const KState*, int32_t, int32_t, int32_t*, int32_t*, hipStream_t);
hipError_t lrl_launch_set_root(const KState*, const float*, const int32_t*, int32_t, hipStream_t);
hipError_t lrl_launch_step_code(const KState*, int32_t, int32_t, int32_t, float*, int32_t*, hipStream_t);
hipError_t lrl_launch_apply_commands(const KState*, int32_t, const int32_t*, int32_t, const float*, const float*, float*,
                                     int32_t, hipStream_t);
hipError_t lrl_launch_terrain_curriculum(const KState*, const int32_t*, int32_t, const int32_t*, int64_t*, const int64_t*,
                                         const int64_t*, const float*, int32_t, int32_t, float, float, int32_t, int64_t,
                                         hipStream_t);
hipError_t lrl_launch_set_dof(const KState*, const float*, const float*, const int32_t*, int32_t, hipStream_t);
hipError_t lrl_launch_rigid_body(const KParams*, const KState*, const int32_t*, const int32_t*, const float*,
                                 hipStream_t);
hipError_t lrl_launch_extras_snapshot(const KParams*, const KState*, const int32_t*, const int32_t*, const float*, float*,
                                      hipStream_t);
hipError_t lrl_launch_shift_history(const KState*, int, int, int, int, hipStream_t);
hipError_t lrl_launch_garbage(uint32_t mode, uint32_t pat, hipStream_t st);
hipError_t lrl_launch_randomize(const KState*, int32_t, int32_t, const float*, const float*, const float*, const float*,
                                uint32_t, hipStream_t);
// lrl_curriculum_dev.hip, lrl_render.hip, lrl_metrics.hip
hipError_t lrl_launch_curriculum_dev(const lrl_dev_curriculum*, const KState*, int32_t, const int32_t*, int32_t,
                                     const int32_t*, int32_t, int32_t, int32_t, double, double, double, int32_t,
                                     int32_t, hipStream_t);
hipError_t lrl_launch_render(const KParams*, const KState*, const KRender*, const lrl_camera*, int32_t, uint8_t*, float*,
                             int32_t*, const int32_t*, hipStream_t);
hipError_t lrl_launch_record_state(const KState*, int32_t, int32_t, int32_t*, hipStream_t);
// lrl_depth.hip: num_envs workgroups, image b of env first_env + b
hipError_t lrl_launch_depth(const KParams*, const KState*, const KRender*, const lrl_depth_camera*, int32_t, int32_t,
                            int32_t, float*, int32_t*, hipStream_t);
// lrl_depth_sense.hip: num_envs workgroups, row b of every array of env first_env + b
hipError_t lrl_launch_depth_sense(const KState*, const lrl_depth_sensor*, int32_t, int32_t, int32_t, uint64_t,
                                  const float*, const float*, float*, int32_t*, int32_t*, float*, hipStream_t);
hipError_t lrl_launch_metrics(const KParams*, const KState*, const KMetrics*, int, hipStream_t);
hipError_t lrl_launch_metrics_clear(const KState*, const KMetrics*, hipStream_t);
hipError_t lrl_launch_metrics_reduce(const KParams*, const KState*, const KMetrics*, int32_t, int32_t, double*,
                                     hipStream_t);
// lrl_nav.hip (hist_floats: one env's row of the observation history)
hipError_t lrl_launch_nav_begin(const KState*, const lrl_nav_state*, const float*, hipStream_t);
hipError_t lrl_launch_nav_flags(const KState*, const lrl_nav_state*, hipStream_t);
hipError_t lrl_launch_nav_log(const KState*, const lrl_nav_state*, int32_t, hipStream_t);
hipError_t lrl_launch_nav_finish(const KState*, const lrl_nav_state*, int32_t, hipStream_t);
}
