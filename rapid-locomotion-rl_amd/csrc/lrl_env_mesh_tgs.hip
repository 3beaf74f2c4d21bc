// lrl_env_mesh_tgs.hip — the terrain-mesh TGS build of the env step kernel (lrl_env_builds::mesh_tgs, lrl_env_layout.h):
// the mesh layout with the TGS contact solver instead of PGS (Cfg.sim.physx.terrain_solver_type 1) and the LDS for its
// fields.  This translation unit holds lrl::mesh_tgs::env_step_kernel<true> and the build's entry points; lrl_env_dispatch.hip
// dispatches to them when the sim's parameters ask for TGS on the mesh.
#define LRL_ENV_BUILD mesh_tgs
#include "lrl_env_step.h"
LRL_ENV_ENTRY_POINTS(LRL_ENV_BUILD)
