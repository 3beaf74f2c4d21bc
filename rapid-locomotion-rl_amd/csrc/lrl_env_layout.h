// The builds of the env step kernel and the map of its dynamic LDS, shared by the kernel (lrl_env_step.h) and the
// host (lrl_capi.cpp::lrl_sim_create takes the launch's LDS byte count from it).  Plain C++: g++ compiles it
// (tests/test_env_lds_layout.py).
#pragma once
#include "lrl_kparams.h"

#ifdef __HIPCC__
#define LRL_LAYOUT_FN __host__ __device__
#else
#define LRL_LAYOUT_FN
#endif

// A build of the env step kernel (lrl_env_step.h describes the lane layouts).
enum lrl_env_solver { LRL_ENV_PGS = 0, LRL_ENV_PGS_OR_TGS = 1, LRL_ENV_TGS = 2 };
struct lrl_env_build {
  bool terrain;     // terrain mesh (env_step_kernel<true>) or ground plane (env_step_kernel<false>)
  int envs;         // envs per workgroup
  int solver;       // lrl_env_solver
  const char* ns;   // the inline namespace the build's kernel lives in (part of its symbol name)
  // quads per env
  constexpr int mirror() const { return LRL_ENV_LANES / (4 * envs); }
  // LDS fields per leg block (map above Lds in lrl_env_step.h): the builds with TGS carry the leg's accumulated
  // joint-space motion dz (fields 51..53); the mesh PGS build does not (its 16-env workgroup fills the CU's LDS)
  constexpr int legf() const { return solver == LRL_ENV_PGS ? 51 : 54; }
  // LDS fields per contact-sphere row (map above contact_setup): the plane build's last field is the TGS solver's
  // restitution target; the mesh TGS build keeps the targets out of the rows, in LDS that is dead during the solve
  // (lrl_env_lds::br)
  constexpr int nsf() const { return terrain ? 67 : 68; }
};
namespace lrl_env_builds {
constexpr lrl_env_build plane = {false, LRL_ENV_LANES / 16, LRL_ENV_PGS_OR_TGS, "flat"};
constexpr lrl_env_build mesh = {true, LRL_ENV_LANES / 4, LRL_ENV_PGS, "mesh"};
constexpr lrl_env_build mesh_tgs = {true, LRL_ENV_LANES / 4, LRL_ENV_TGS, "mesh_tgs"};
}  // namespace lrl_env_builds
#define LRL_ENV_BUILDS(X) X(plane) X(mesh) X(mesh_tgs)
// the namespaces as tokens, for the one place that has to paste them (lrl_env_step.h; it checks them against ns)
#define LRL_ENV_NS_plane flat
#define LRL_ENV_NS_mesh mesh
#define LRL_ENV_NS_mesh_tgs mesh_tgs

constexpr bool lrl_str_eq(const char* a, const char* b) { return *a == *b && (*a == 0 || lrl_str_eq(a + 1, b + 1)); }
// only the three combinations above exist
constexpr bool lrl_env_build_known(const lrl_env_build& b) {
#define LRL_X(k) \
  (b.terrain == lrl_env_builds::k.terrain && b.envs == lrl_env_builds::k.envs && b.solver == lrl_env_builds::k.solver && \
   lrl_str_eq(b.ns, lrl_env_builds::k.ns)) ||
  return LRL_ENV_BUILDS(LRL_X) false;
#undef LRL_X
}

#define LRL_LIMF 19  // LDS fields per joint-limit row (map above limit_setup)
#define LRL_KLEGF ((int)(sizeof(KLeg) / sizeof(float)))  // floats of one leg's model table

// The kernel's dynamic LDS, as offsets in floats from its start (bytes: the whole).  Rows are [field][env slot]
// columns: field f of a row at offset o is o + f * envs + the lane's env slot.
//   leg       4 leg blocks of legf() fields
//   sph       num_spheres contact rows of nsf() fields
//   scratch   the terrain query's scratch: the vertex blocks (float4 [16][lanes]); on the plane only the limit rows.
//             mesh TGS: the vertex blocks, then the query work list at the scratch's tail (5 floats per lane: candidate
//             masks, offsets, and from `hit` the masks of the candidates found in contact, which the activation reads)
//   lim       12 joint-limit rows of LRL_LIMF fields: their own region on the plane; on the mesh they alias the start
//             of the scratch once a sub-step's queries are done
//   br        (mesh TGS) restitution targets [sphere][env slot] after the limit rows: they may run over the dead part of
//             the work list but not over the hit masks, so a model with more spheres than that leaves room for gets a
//             longer scratch.  (plane: the row's last field; mesh PGS: none)
//   ktab      model tables staged once per launch: KParams::leg[4], per sphere (x, y, z, radius), per sphere its link
//   sgrp      self-collision groups [lane][g][begin, end) (KParams::self_grp), then from spair the pairs
//   wl        the query work list: mesh PGS after the tables (at an even offset: its masks are 64-bit); mesh TGS inside
//             the scratch; the plane has none
//   otile, ptile, rtile   after the physics the front is reused: obs rows [envs][num_obs], privileged rows
//             [envs][LRL_NUM_PRIV], reward-term rows [envs][LRL_MAX_REWARD_TERMS]
struct lrl_env_lds {
  int leg, sph, scratch, lim, br, hit, ktab, sgrp, spair, wl, otile, ptile, rtile;
  int end_contacts, end_tiles;  // ends of the two uses of the LDS, in floats
  int bytes;
};
LRL_LAYOUT_FN constexpr lrl_env_lds lrl_env_lds_layout(const lrl_env_build& b, int num_spheres, int self_npairs, int num_obs) {
  const int lanes = LRL_ENV_LANES, envs = b.envs, tgs = b.terrain && b.solver == LRL_ENV_TGS;
  lrl_env_lds L = {};
  L.leg = 0;
  L.sph = 4 * b.legf() * envs;
  L.scratch = (4 * b.legf() + num_spheres * b.nsf()) * envs;
  L.lim = L.scratch;
  const int rows_and_hits = (LRL_NUM_DOF * LRL_LIMF + num_spheres) * envs + 2 * lanes;
  const int scratch_len = tgs          ? ((64 + 5) * lanes > rows_and_hits ? (64 + 5) * lanes : rows_and_hits)
                          : b.terrain ? 64 * lanes
                                      : LRL_NUM_DOF * LRL_LIMF * envs;
  L.ktab = L.scratch + scratch_len;
  L.br = tgs ? L.lim + LRL_NUM_DOF * LRL_LIMF * envs : -1;
  L.hit = tgs ? L.ktab - 2 * lanes : -1;
  L.sgrp = L.ktab + 4 * LRL_KLEGF + 5 * num_spheres;
  L.spair = L.sgrp + 40;
  const int tables = 4 * LRL_KLEGF + 5 * num_spheres + 40 + self_npairs + 1;  // (+ 1: room to round wl up)
  L.wl = tgs ? L.ktab - 5 * lanes : b.terrain ? L.ktab + (tables & ~1) : -1;
  L.end_contacts = L.ktab + tables + (b.terrain && !tgs ? 5 * lanes : 0);
  L.otile = 0;
  L.ptile = envs * num_obs;
  L.rtile = envs * (num_obs + LRL_NUM_PRIV);
  L.end_tiles = envs * (num_obs + LRL_NUM_PRIV + LRL_MAX_REWARD_TERMS);
  L.bytes = 4 * (L.end_contacts > L.end_tiles ? L.end_contacts : L.end_tiles);
  return L;
}
