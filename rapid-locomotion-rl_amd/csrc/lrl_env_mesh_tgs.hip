// lrl_env_mesh_tgs.hip — the terrain-mesh TGS build of the env step kernel: lrl_env.hip's mesh layout (16 envs per
// single-wave workgroup) with the TGS contact solver instead of PGS (Cfg.sim.physx.terrain_solver_type 1; the LDS for
// its fields: lrl_kparams.h).  Only env_step_kernel<true> and its entry points (lrl_launch_env_step_mesh_tgs,
// lrl_env_kernel_setup_mesh_tgs, lrl_debug_env_profile_mesh_tgs, lrl_debug_env_buffer_mesh_tgs) come from this
// translation unit; lrl_env.hip's lrl_launch_env_step dispatches to it, and its PGS mesh kernel is built as before.
#define LRL_ENV_MESH_TGS_TU
#include "lrl_env.hip"
