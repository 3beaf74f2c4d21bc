"""CPU-side checks of the env step kernel's LDS map (csrc/lrl_env_layout.h), the one function the kernel addresses its
LDS with and lrl_sim_create sizes the launch with: a stand-alone program built with g++ prints every region offset
and the total for the three builds over a grid of models, and the test checks the total against the sum the host
used to form by hand, that regions live at the same time do not overlap, and the mesh TGS build's margin."""
import itertools
import os
import subprocess

import pytest

from lrl.robot import load_robot

from helpers import ROBOT_FILES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rapid-locomotion-rl_amd", "csrc")

# include/lrl.h, csrc/lrl_kparams.h
LANES, MAX_SPHERES, MAX_SELF_PAIRS, MAX_OBS, NUM_DOF, NUM_PRIV, MAX_REWARD_TERMS = 64, 40, 256, 256, 12, 18, 24
KLEGF = 3 * 3 + 3 * 9 + 3 * 3 + 3 + 3 * 3 + 3 * 6  # floats of a KLeg
LIMF = 19
BUILDS = ("plane", "mesh", "mesh_tgs")
FIELDS = ("leg", "sph", "scratch", "lim", "br", "hit", "ktab", "sgrp", "spair", "wl", "otile", "ptile", "rtile",
          "end_contacts", "end_tiles", "bytes")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include "lrl_env_layout.h"
int main(int argc, char** argv) {
  const lrl_env_build bogus = {true, LRL_ENV_LANES / 16, LRL_ENV_PGS, "mesh"};
  printf("consts %d %d %d %d %d %d %d %d %d %d\n", LRL_ENV_LANES, LRL_MAX_SPHERES, LRL_MAX_SELF_PAIRS, LRL_MAX_OBS,
         LRL_NUM_DOF, LRL_NUM_PRIV, LRL_MAX_REWARD_TERMS, LRL_KLEGF, LRL_LIMF, (int)lrl_env_build_known(bogus));
#define BUILD(b) \
  printf("build " #b " %d %d %d %d %d %d %s\n", (int)lrl_env_builds::b.terrain, lrl_env_builds::b.envs, \
         lrl_env_builds::b.solver, lrl_env_builds::b.legf(), lrl_env_builds::b.nsf(),                    \
         (int)lrl_env_build_known(lrl_env_builds::b), lrl_env_builds::b.ns);
  LRL_ENV_BUILDS(BUILD)
  for (int i = 1; i + 2 < argc; i += 3) {
    const int nsph = atoi(argv[i]), npairs = atoi(argv[i + 1]), nobs = atoi(argv[i + 2]);
#define CASE(b)                                                                                                     \
  {                                                                                                                 \
    const lrl_env_lds L = lrl_env_lds_layout(lrl_env_builds::b, nsph, npairs, nobs);                                \
    printf("case " #b " %d %d %d : %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", nsph, npairs, nobs, L.leg,  \
           L.sph, L.scratch, L.lim, L.br, L.hit, L.ktab, L.sgrp, L.spair, L.wl, L.otile, L.ptile, L.rtile,          \
           L.end_contacts, L.end_tiles, L.bytes);                                                                   \
  }
    LRL_ENV_BUILDS(CASE)
  }
  return 0;
}
"""


def _preset_spheres():
    return {r: load_robot(f)["num_spheres"] for r, f in ROBOT_FILES.items()}


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """(build descriptions, {(build, nsph, npairs, nobs): {field: value}}) as the header computes them."""
    d = tmp_path_factory.mktemp("lds_layout")
    exe, src = str(d / "lds_layout"), str(d / "lds_layout.cpp")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, src])
    grid = itertools.product(sorted(set(_preset_spheres().values()) | {MAX_SPHERES}), (0, 37, MAX_SELF_PAIRS),
                             (42, 235, MAX_OBS))
    args = [str(v) for case in grid for v in case]
    builds, cases = {}, {}
    for line in subprocess.check_output([exe] + args).decode().splitlines():
        w = line.split()
        if w[0] == "consts":
            assert [int(x) for x in w[1:]] == [LANES, MAX_SPHERES, MAX_SELF_PAIRS, MAX_OBS, NUM_DOF, NUM_PRIV,
                                               MAX_REWARD_TERMS, KLEGF, LIMF, 0]  # (last: a fourth build is refused)
        elif w[0] == "build":
            builds[w[1]] = dict(zip(("terrain", "envs", "solver", "legf", "nsf", "known"), map(int, w[2:8])), ns=w[8])
        else:
            cases[(w[1], int(w[2]), int(w[3]), int(w[4]))] = dict(zip(FIELDS, map(int, w[6:])))
    assert set(builds) == set(BUILDS) and len(cases) == 3 * len(args) // 3
    return builds, cases


def test_three_builds(layout):
    builds, _ = layout
    assert all(b["known"] == 1 for b in builds.values())
    assert {k: (b["terrain"], b["envs"], b["solver"], b["ns"]) for k, b in builds.items()} == {
        "plane": (0, LANES // 16, 1, "flat"), "mesh": (1, LANES // 4, 0, "mesh"),
        "mesh_tgs": (1, LANES // 4, 2, "mesh_tgs")}


def _parent_bytes(build, nsph, npairs, nobs):
    """lrl_sim_create's byte count before the layout function existed, term by term."""
    terrain, tgs = build != "plane", build == "mesh_tgs"
    wg_envs = LANES // 4 if terrain else LANES // 16
    legf = 54 if tgs else 51 if terrain else 54
    nsf = 67 if terrain else 68
    contacts = (4 * legf + nsph * nsf) * wg_envs * 4
    tgs_scratch = max((64 + 5) * LANES, (NUM_DOF * LIMF + nsph) * (LANES // 4) + 2 * LANES)
    contacts += tgs_scratch * 4 if tgs else 16 * LANES * 16 if terrain else NUM_DOF * LIMF * wg_envs * 4
    contacts += (4 * KLEGF + 5 * nsph) * 4
    contacts += (40 + npairs + 1) * 4
    if terrain and not tgs:
        contacts += LANES * 20
    tiles = (nobs + NUM_PRIV + MAX_REWARD_TERMS) * wg_envs * 4
    return max(contacts, tiles)


def test_total_is_the_former_host_sum(layout):
    _, cases = layout
    for (build, nsph, npairs, nobs), L in cases.items():
        assert L["bytes"] == _parent_bytes(build, nsph, npairs, nobs), (build, nsph, npairs, nobs, L)
        assert L["bytes"] == 4 * max(L["end_contacts"], L["end_tiles"])


def _disjoint(regions, what):
    """regions: (name, begin, end) in floats; no two overlap."""
    rs = sorted(regions, key=lambda r: r[1])
    for (na, a0, a1), (nb, b0, b1) in zip(rs, rs[1:]):
        assert a0 <= a1 <= b0 <= b1, (what, na, a0, a1, nb, b0, b1)


def test_live_regions_do_not_overlap(layout):
    builds, cases = layout
    for key, L in cases.items():
        build, nsph, npairs, nobs = key
        B = builds[build]
        envs, total = B["envs"], L["bytes"] // 4
        legs = ("leg", L["leg"], L["leg"] + 4 * B["legf"] * envs)
        rows = ("sph", L["sph"], L["sph"] + nsph * B["nsf"] * envs)
        scratch = ("scratch", L["scratch"], L["ktab"])
        tables = [("ktab", L["ktab"], L["sgrp"]), ("sgrp", L["sgrp"], L["spair"]),
                  ("spair", L["spair"], L["spair"] + npairs)]
        assert L["sgrp"] - L["ktab"] == 4 * KLEGF + 5 * nsph and L["spair"] - L["sgrp"] == 40
        lim = ("lim", L["lim"], L["lim"] + NUM_DOF * LIMF * envs)
        # the whole physics: leg blocks, contact rows, the scratch, the staged tables (+ the PGS mesh work list)
        phys = [legs, rows, scratch] + tables
        if build == "mesh":
            assert L["wl"] % 2 == 0  # 64-bit masks
            phys.append(("wl", L["wl"], L["wl"] + 5 * LANES))
        else:
            assert build == "mesh_tgs" or L["wl"] == -1
        _disjoint(phys, key)
        assert max(r[2] for r in phys) <= L["end_contacts"] <= total  # (the tables carry one float of padding)
        # inside the scratch
        assert scratch[1] <= lim[1] and lim[2] <= scratch[2], (key, lim, scratch)
        if build == "plane":
            assert (lim[1], lim[2]) == (scratch[1], scratch[2]) and L["br"] == -1 and L["hit"] == -1
        else:
            verts = ("verts", L["scratch"], L["scratch"] + 64 * LANES)
            assert lim[1] == verts[1] and lim[2] <= verts[2]  # the limit rows alias the (dead) vertex blocks
            if build == "mesh":
                assert verts[2] == scratch[2] and L["br"] == -1 and L["hit"] == -1
            else:
                # during the queries: vertex blocks and the work list (its last 2 floats per lane: the hit masks)
                wl = ("wl", L["wl"], L["wl"] + 5 * LANES)
                assert wl[2] == scratch[2] and L["hit"] == wl[2] - 2 * LANES
                _disjoint([verts, wl], key)
                # during the solve: limit rows, restitution targets and the hit masks the activation still reads
                br = ("br", L["br"], L["br"] + nsph * envs)
                hit = ("hit", L["hit"], L["hit"] + 2 * LANES)
                assert br[1] == lim[2] and br[2] <= hit[1], (key, br, hit)
                _disjoint([lim, br, hit], key)
        # after the physics: the tiles over the front
        tiles = [("otile", L["otile"], L["otile"] + envs * nobs), ("ptile", L["ptile"], L["ptile"] + envs * NUM_PRIV),
                 ("rtile", L["rtile"], L["rtile"] + envs * MAX_REWARD_TERMS)]
        _disjoint(tiles, key)
        assert L["otile"] == 0 and tiles[-1][2] == L["end_tiles"] <= total


def test_mesh_tgs_costs_the_dz_fields(layout):
    """Each preset's mesh TGS build takes the PGS build's LDS plus the twelve dz leg fields of its 16 envs (the fact
    test_terrain_tgs_gpu.py::test_mesh_tgs_lds_fits reads back from a sim)."""
    _, cases = layout
    for nsph in _preset_spheres().values():
        for npairs, nobs in itertools.product((0, 37, MAX_SELF_PAIRS), (42, 235, MAX_OBS)):
            tgs, pgs = cases[("mesh_tgs", nsph, npairs, nobs)]["bytes"], cases[("mesh", nsph, npairs, nobs)]["bytes"]
            assert tgs - pgs == 12 * 16 * 4, (nsph, npairs, nobs, pgs, tgs)
