// lrl_env_mesh.hip — the terrain-mesh build of the env step kernel (lrl_env_builds::mesh, lrl_env_layout.h): one quad
// per env, 16 envs per single-wave workgroup, PGS contact solver.  This translation unit holds
// lrl::mesh::env_step_kernel<true> and the build's entry points; lrl_env_dispatch.hip dispatches to them.
#define LRL_ENV_BUILD mesh
#include "lrl_env_step.h"
LRL_ENV_ENTRY_POINTS(LRL_ENV_BUILD)
