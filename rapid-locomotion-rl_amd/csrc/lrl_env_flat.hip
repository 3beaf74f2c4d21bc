// lrl_env_flat.hip — the plane build of the env step kernel (lrl_env_builds::plane, lrl_env_layout.h): 4 envs per
// single-wave workgroup, 16 lanes (4 mirrored quads) per env; PGS, or TGS by KParams::p.solver_tgs.  This translation
// unit holds lrl::flat::env_step_kernel<false> and the build's entry points; lrl_env_dispatch.hip dispatches to them.
#define LRL_ENV_BUILD plane
#include "lrl_env_step.h"
LRL_ENV_ENTRY_POINTS(LRL_ENV_BUILD)
