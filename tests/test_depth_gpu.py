"""The egocentric depth camera on cuda:0 (lrl_sim_depth, and LeggedRobotEnv with the Cfg.depth group) against the numpy
checker tests/depth_ref.py, which tests/test_depth_ref.py pins on analytic scenes.

Pass rule of every image comparison (conditions, not measurements; the ids rule is tests/test_render_gpu.py's): the
checker alone, float32 against float64, may disagree in `ids` on at most 0.25 % of the scene's pixels; the kernel may
then disagree with the float64 checker on at most 0.5 %, and every disagreeing pixel has another id among its 8
neighbours in the checker's image.  On quiet pixels (ids agree, off every id edge, the reference not within the bar of
near or far; on the terrain mesh also depth_ref.quiet_ground's, which finds ground-on-ground occlusion edges from the
reference alone) depths are within DEPTH_REL_BAR of the float64 checker's, and where the reference clamps to near or
far the kernel's value is bit-equal to near / far.

DEPTH_REL_BAR: 4 x the worst |z - z64| / z64 measured on an MI355X over all scenes of this file (the plane scenes of
every image size and both mounts, and the four terrain scenes), the headroom DESIGN.md §3 gives a compiler change.  The
measured figure stands beside the constant.  As a guard against a wrong kernel setting its own bar, that worst error may
be at most 16 x the worst float32-checker-vs-float64-checker error over the same pixels.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import depth_ref as dr
import depth_scenes as ds
import render_ref as rr
from lrl import _abi
from lrl import config as lcfg

pytestmark = pytest.mark.gpu

# Measured on an MI355X over the 34 images of this file: kernel 1.439e-6 (terrain scene 2, the base 31 m from the world
# origin: the rounding of o = p + R pos at that distance), float32 checker 1.561e-6 on the same pixels; the plane scenes
# (bases within 5 m of the origin) stay under 3.93e-7 (float32 checker 3.92e-7).
DEPTH_REL_BAR = 4 * 1.439e-6
DEV = "cuda:0"
MOUNT = dict(pos=(0.27, 0.0, 0.03), pitch_deg=20.0)   # add_depth_camera's default: ahead of the trunk, sees no robot
CHASE = dict(pos=(-0.55, 0.05, 0.35), pitch_deg=30.0)  # behind and above the trunk: the robot fills the image
WORST = {}  # label -> (kernel's worst relative error on quiet pixels, the float32 checker's on the same pixels)


def _mc_cfg(n):
    cfg = lcfg.make_cfg()
    lcfg.config_mini_cheetah(cfg)
    cfg.env.num_envs = n
    return cfg


def _model(env):
    M = env._M
    return dict(num_bodies=M.num_bodies, num_spheres=M.num_spheres, body_leg=np.array(M.body_leg[:]),
                body_link=np.array(M.body_link[:]), sphere_body=np.array(M.sphere_body[:]),
                sphere_pos=np.array(M.sphere_pos, np.float32).reshape(_abi.MAX_SPHERES, 3),
                sphere_radius=np.array(M.sphere_radius[:], np.float32))


def _camera(width, height, see_robot=True, hfov_deg=87.0, near=0.05, far=3.0, pos=MOUNT["pos"],
            pitch_deg=MOUNT["pitch_deg"], **_):
    cam = _abi.LrlDepthCamera()
    cam.pos[:] = [float(x) for x in pos]
    cam.pitch_deg, cam.hfov_deg, cam.near, cam.far = pitch_deg, hfov_deg, near, far
    cam.width, cam.height = width, height
    cam.flags = 0 if see_robot else _abi.DEPTH_NO_ROBOT
    return cam


def _cam_dict(cam):
    """The camera as the kernel holds it: the struct's float32 fields."""
    return dict(pos=np.array(cam.pos[:], np.float32), pitch_deg=np.float32(cam.pitch_deg),
                hfov_deg=np.float32(cam.hfov_deg), near=np.float32(cam.near), far=np.float32(cam.far),
                width=cam.width, height=cam.height)


def _depth(env, cam, first=0, count=None, only_reset=0, depth=None, ids=None):
    """lrl_sim_depth on envs [first, first + count) into fresh (or the given) device buffers; returns (rc, depth, ids)."""
    count = env.num_envs - first if count is None else count
    if depth is None:
        depth = torch.full((max(count, 0), cam.height, cam.width), -7.0, device=DEV)
    if ids is None:
        ids = torch.full((max(count, 0), cam.height, cam.width), -7, dtype=torch.int32, device=DEV)
    rc = _abi.lib().lrl_sim_depth(env._sim, C.byref(cam), first, count, only_reset, C.c_void_p(depth.data_ptr()),
                                  C.c_void_p(ids.data_ptr()), env._stream())
    torch.cuda.synchronize()
    return rc, depth, ids


def _judge(label, kz, kid, r64, r32, cam, quiet_extra=None):
    """Apply the pass rule to one image; records the worst relative errors in WORST and returns them."""
    npx = cam.width * cam.height
    near, far = np.float32(cam.near), np.float32(cam.far)
    self_bad = int((r32["ids"] != r64["ids"]).sum())
    bad = kid != r64["ids"]
    edge = rr.boundary(r64["ids"])
    z = r64["depth"]
    inner = (z > float(near) * (1 + DEPTH_REL_BAR)) & (z < float(far) * (1 - DEPTH_REL_BAR))
    quiet = ~bad & ~edge & (r64["ids"] > 0) & inner
    loud = 0
    if quiet_extra is not None:
        loud = int((quiet & ~quiet_extra).sum())
        quiet &= quiet_extra
    q32 = quiet & (r32["ids"] == r64["ids"])
    rel = float((np.abs(kz.astype(np.float64) - z) / z)[quiet].max()) if quiet.any() else 0.0
    rel32 = float((np.abs(r32["depth"].astype(np.float64) - z) / z)[q32].max()) if q32.any() else 0.0
    WORST[label] = (rel, rel32)
    print(f"{label}: {npx} px, checker f32 vs f64 ids {self_bad}, kernel vs f64 ids {int(bad.sum())} "
          f"(off an edge {int((bad & ~edge).sum())}), quiet {int(quiet.sum())}, not quiet ground {loud}, "
          f"max rel depth err kernel {rel:.3e} / f32 checker {rel32:.3e}")
    assert self_bad <= 0.0025 * npx, (label, self_bad)
    assert bad.sum() <= 0.005 * npx, (label, int(bad.sum()))
    assert not np.any(bad & ~edge), (label, np.argwhere(bad & ~edge)[:5])
    clamp_far = ~bad & (z == np.float64(far))
    clamp_near = ~bad & (z == np.float64(near))
    assert np.all(kz[clamp_far].view(np.uint32) == far.view(np.uint32)), label
    assert np.all(kz[clamp_near].view(np.uint32) == near.view(np.uint32)), label
    assert np.all(kz[kid == 0].view(np.uint32) == far.view(np.uint32)), label
    assert np.all((kz >= near) & (kz <= far)), label
    assert rel < DEPTH_REL_BAR, (label, rel)
    return rel, rel32


@pytest.fixture(scope="module")
def mc_env():
    from lrl.env import LeggedRobotEnv
    env = LeggedRobotEnv(DEV, cfg=_mc_cfg(5), seed=2)  # 5 envs: the SoA padding to 64 is in play
    env.reset()
    assert not hasattr(env, "depth_images")  # no depth group: no buffer
    # five distinct base poses: roll, pitch and yaw all non-zero, different heights
    rpy = [(12.0, -8.0, 35.0), (-20.0, 10.0, 160.0), (6.0, 22.0, -100.0), (-9.0, -15.0, 250.0), (25.0, 5.0, -30.0)]
    xyz = [(0.7, -1.3, 0.32), (2.1, 0.4, 0.45), (-1.6, 2.2, 0.28), (3.3, 3.1, 0.60), (-2.4, -0.9, 0.38)]
    q = np.stack([ds.quat_rpy(*a) for a in rpy])
    env.root_states[:, 3:7] = torch.tensor(q, device=DEV)
    env.root_states[:, 0:3] = torch.tensor(xyz, device=DEV)
    torch.cuda.synchronize()
    yield env
    env.close()


PLANE_SCENES = [  # (width, height, mount, see_robot)
    (1, 1, CHASE, True), (1, 1, MOUNT, False),
    (16, 16, MOUNT, True), (16, 16, CHASE, False),      # exactly one pass of 256
    (33, 17, CHASE, True), (33, 17, MOUNT, False),      # 561 pixels: three passes, a ragged tail, W no multiple of 16
]


@pytest.fixture(scope="module")
def plane_images(mc_env):
    """Every plane scene, all five envs in one launch each, with the checker's float64 and float32 images (computed
    once, shared by the tests below)."""
    env, out = mc_env, []
    model = _model(env)
    for w, h, mount, robot in PLANE_SCENES:
        cam = _camera(w, h, see_robot=robot, **mount)
        rc, kz, kid = _depth(env, cam)
        assert rc == 0, _abi.lib().lrl_last_error()
        rb = env.rigid_body_state.cpu().numpy()  # (the call refreshed it)
        cd = _cam_dict(cam)
        for e in range(env.num_envs):
            prims = rr.scene_from_state(rb[e], model) if robot else None
            r64 = dr.trace(prims, ("plane",), rb[e, 0, 0:3], rb[e, 0, 3:7], cd, np.float64)
            r32 = dr.trace(prims, ("plane",), rb[e, 0, 0:3], rb[e, 0, 3:7], cd, np.float32)
            label = f"plane {w}x{h} {'chase' if mount is CHASE else 'mount'} {'robot' if robot else 'no robot'} env {e}"
            out.append((label, kz[e].cpu().numpy(), kid[e].cpu().numpy(), r64, r32, cam))
    return out


def test_plane_mini_cheetah_images(mc_env, plane_images):
    rb = mc_env.rigid_body_state.cpu().numpy()
    assert len({round(float(z), 3) for z in rb[:, 0, 2]}) == 5  # the five bases are where the fixture put them
    seen, sizes = set(), set()
    for label, kz, kid, r64, r32, cam in plane_images:
        _judge(label, kz, kid, r64, r32, cam)
        seen |= set(r64["ids"].ravel().tolist())
        sizes.add(kz.shape)
        if cam.flags & _abi.DEPTH_NO_ROBOT:
            assert set(np.unique(kid)) <= {0, rr.ID_GROUND}
    assert sizes == {(1, 1), (16, 16), (17, 33)}
    # the scenes are not empty: nothing-within-far, ground, the base box or a sphere, and a link capsule were compared
    assert {0, rr.ID_GROUND} <= seen
    assert any(rr.ID_BOX <= i < rr.ID_CAPSULE0 for i in seen) and any(i >= rr.ID_CAPSULE0 for i in seen)
    # the five envs' images differ (each is drawn from its own base)
    big = [kz for label, kz, *_ in plane_images if kz.shape == (17, 33) and "chase robot" in label]
    assert len(big) == 5 and all(np.any(big[0] != b) for b in big[1:])


@pytest.fixture(scope="module")
def terrain_images():
    """The four terrain scenes (tests/depth_scenes.py) on the Go1 rough trimesh, drawn with LRL_DEPTH_NO_ROBOT."""
    from lrl.env import LeggedRobotEnv
    cfg = ds.go1_trimesh_cfg()
    env = LeggedRobotEnv(DEV, cfg=cfg, seed=ds.TERRAIN_SEED)
    out = []
    try:
        env.reset()
        assert env._P.terrain_mesh == 1
        vtx = ds.terrain_vertices(cfg)
        rows, cols = env.terrain.heightsamples.shape
        np.testing.assert_array_equal(np.array(env.terrain.vertices, np.float32).reshape(rows, cols, 3)[..., 2],
                                      vtx[..., 2].astype(np.float32))  # the host rebuild is the env's terrain
        for e, sc in ds.TERRAIN_SCENES.items():
            env.root_states[e, 0:3] = torch.tensor(sc["pos"], device=DEV)
            env.root_states[e, 3:7] = torch.tensor(ds.quat_rpy(*sc["rpy"]), device=DEV)
        for e, sc in ds.TERRAIN_SCENES.items():
            cd = ds.terrain_camera(sc["cam"])
            cam = _camera(see_robot=False, **cd)
            rc, kz, kid = _depth(env, cam, first=e, count=1)
            assert rc == 0, _abi.lib().lrl_last_error()
            rb = env.rigid_body_state[e, 0].cpu().numpy()
            np.testing.assert_array_equal(rb[0:3], np.float32(sc["pos"]))
            cd = _cam_dict(cam)
            # brute force over every triangle a ray can reach (a corner ray is longer than far: far is the planar distance)
            ground = ("tris", rr.grid_triangles(vtx, rb[0:3], ds.reach(cd) + 4 * cfg.terrain.horizontal_scale))
            r64, quiet = dr.quiet_ground(ground, rb[0:3], rb[3:7], cd)
            r32 = dr.trace(None, ground, rb[0:3], rb[3:7], cd, np.float32)
            out.append((f"terrain scene {e}", kz[0].cpu().numpy(), kid[0].cpu().numpy(), r64, r32, cam, quiet))
    finally:
        env.close()
    return out


def test_trimesh_go1_images(terrain_images):
    assert len(terrain_images) == 4
    for label, kz, kid, r64, r32, cam, quiet in terrain_images:
        assert kz.shape == (16, 24)
        _judge(label, kz, kid, r64, r32, cam, quiet_extra=quiet)
        g = r64["ids"] == rr.ID_GROUND
        assert g.sum() > 0 and quiet.sum() >= 0.75 * g.sum(), label  # (test_depth_ref.py asserts it on the CPU)
    far_px = [int((kid == 0).sum()) for _, _, kid, *_ in terrain_images]
    assert far_px[0] > 0.25 * 384  # rays leave the grid
    assert far_px[1] > 0.5 * 384   # far = 0.5


def test_depth_accuracy_over_all_scenes(plane_images, terrain_images):
    """The bar and its guard over every scene of this file (the per-image assertions are in _judge)."""
    for label, kz, kid, r64, r32, cam in plane_images:
        _judge(label, kz, kid, r64, r32, cam)
    for label, kz, kid, r64, r32, cam, quiet in terrain_images:
        _judge(label, kz, kid, r64, r32, cam, quiet_extra=quiet)
    worst = max(v[0] for v in WORST.values())
    worst32 = max(v[1] for v in WORST.values())
    at = max(WORST, key=lambda k: WORST[k][0])
    print(f"worst relative depth error over {len(WORST)} images: kernel {worst:.3e} ({at}), "
          f"float32 checker {worst32:.3e}; bar {DEPTH_REL_BAR:.3e}")
    assert len(WORST) == 5 * len(PLANE_SCENES) + 4
    assert worst < DEPTH_REL_BAR
    assert worst <= 16 * worst32, (worst, worst32)


def _depth_env(n, interval, device_resets, seed=7, depth=True, w=16, h=12):
    from lrl.env import LeggedRobotEnv
    cfg = _mc_cfg(n)
    if depth:
        lcfg.add_depth_camera(cfg, width=w, height=h, update_interval=interval, **CHASE)
    env = LeggedRobotEnv(DEV, cfg=cfg, seed=seed, legacy_fork=False, device_resets=device_resets)
    env.reset()
    return env


@pytest.mark.parametrize("device_resets", [True, False])
def test_step_hookup(device_resets):
    env = _depth_env(5, 3, device_resets)
    try:
        assert env._dev_path == device_resets
        assert env.depth_images.shape == (5, 12, 16) and env.depth_images.dtype == torch.float32
        assert env.depth_images.device == env.device and env._depth_step == 1  # (reset() took the first step)
        buf = env.depth_images.data_ptr()
        forced, _ = env.render_depth()
        assert forced is env.depth_images
        gen = torch.Generator(device=DEV).manual_seed(11)
        stale, flagged = 0, 0
        for k in range(1, 8):
            if k == 4:  # an off-interval step: env 2 runs into its time-out in it
                env.episode_length_buf[2] = int(env.max_episode_length)
            prev = env.depth_images.clone()
            _, _, done, _ = env.step(torch.rand(5, 12, device=DEV, generator=gen) * 2 - 1)
            cur, flag = env.depth_images.clone(), done.clone()
            forced = env.render_depth()[0].clone()
            env.depth_images.copy_(cur)  # (the forced refresh is this test's probe, not part of the rollout)
            assert env.depth_images.data_ptr() == buf
            if k == 4:
                assert bool(flag[2])
            if k % 3 == 0:
                assert torch.equal(cur, forced), k
            else:
                assert torch.equal(cur[~flag], prev[~flag]), k
                assert torch.equal(cur[flag], forced[flag]), k
                stale += int((cur[~flag] != forced[~flag]).any())
                flagged += int(flag.sum())
                if bool(flag.any()):
                    assert not torch.equal(cur[flag], prev[flag]), k  # the reset env's image is the new episode's
        assert stale >= 3 and flagged >= 1  # the held images were really out of date, and a flagged env was redrawn
        d, ids = env.render_depth(ids=True)
        assert ids.dtype == torch.int32 and ids.shape == d.shape and int(ids.max()) >= rr.ID_BOX
    finally:
        env.close()


def test_rollout_is_unchanged_by_the_sensor():
    a, b = _depth_env(5, 2, None, seed=9), _depth_env(5, 2, None, seed=9, depth=False)
    try:
        assert not hasattr(b, "depth_images") and b._depth_cam is None
        with pytest.raises(RuntimeError, match="add_depth_camera"):
            b.render_depth()
        gen = torch.Generator(device=DEV).manual_seed(13)
        for _ in range(5):
            act = torch.rand(5, 12, device=DEV, generator=gen) * 2 - 1
            oa, ra, da, xa = a.step(act)
            ob, rb, db, xb = b.step(act)
            for x, y in ((oa, ob), (xa["privileged_obs"], xb["privileged_obs"]), (ra, rb), (da, db),
                         (a.root_states, b.root_states)):
                assert torch.equal(x, y)
    finally:
        a.close()
        b.close()


def test_buffers_and_refusals(mc_env):
    env = mc_env
    L = _abi.lib()
    cam = _camera(16, 12, **CHASE)
    buf = torch.full((5, 12, 16), -7.0, device=DEV)
    idb = torch.full((5, 12, 16), -7, dtype=torch.int32, device=DEV)
    rc, _, _ = _depth(env, cam, first=1, count=3, depth=buf[1:], ids=idb[1:])
    assert rc == 0
    assert bool((buf[0] == -7).all()) and bool((buf[4] == -7).all()) and bool((buf[1:4] > 0).all())
    assert bool((idb[0] == -7).all()) and bool((idb[4] == -7).all()) and bool((idb[1:4] >= 0).all())
    rc, full, _ = _depth(env, cam)
    assert rc == 0 and torch.equal(full[1:4], buf[1:4])  # image b of a range is env first + b's
    rc, again, _ = _depth(env, cam)
    assert rc == 0 and torch.equal(full, again)  # two identical calls: bit-identical images
    # only_reset with no reset flag set: nothing is written
    flags = env._reset_u8.clone()
    env._reset_u8.zero_()
    before = buf.clone()
    rc, _, _ = _depth(env, cam, only_reset=1, depth=buf, ids=idb)
    assert rc == 0 and torch.equal(buf, before)
    env._reset_u8[3] = 1  # ... and with one set, that env's image alone
    rc, _, _ = _depth(env, cam, only_reset=1, depth=buf, ids=idb)
    assert rc == 0 and torch.equal(buf[3], full[3]) and torch.equal(buf[:3], before[:3]) and torch.equal(buf[4], before[4])
    env._reset_u8.copy_(flags)

    # refusals: LRL_E_INVALID, a message, no launch
    poison = torch.full((5, 12, 16), -7.0, device=DEV)
    pid = torch.full((5, 12, 16), -7, dtype=torch.int32, device=DEV)

    def call(sim=True, camera=True, depth=True, first=0, count=5, **kw):
        c = _camera(16, 12, **CHASE)
        for key, v in kw.items():
            setattr(c, key, v)
        return L.lrl_sim_depth(env._sim if sim else None, C.byref(c) if camera else None, first, count, 0,
                               C.c_void_p(poison.data_ptr()) if depth else None, C.c_void_p(pid.data_ptr()),
                               env._stream())
    bad = [dict(sim=False), dict(camera=False), dict(depth=False), dict(first=-1), dict(first=1, count=5),
           dict(first=6, count=0), dict(count=-1), dict(count=6), dict(width=0), dict(width=1025), dict(height=0),
           dict(height=1025), dict(hfov_deg=1.0), dict(hfov_deg=179.0), dict(near=-0.01), dict(near=3.0),
           dict(near=4.0), dict(far=3.0e38), dict(far=float("inf")), dict(far=float("nan")), dict(pitch_deg=90.0),
           dict(pitch_deg=-90.0), dict(pitch_deg=120.0)]
    for kw in bad:
        L.lrl_set_error(0, b"")
        assert call(**kw) == -1, kw
        assert len(L.lrl_last_error()) > 0, kw
    # terrain_mesh set without lrl_sim_set_terrain: a sim of its own (the env's always carries its terrain)
    P = type(env._P).from_buffer_copy(env._P)
    P.terrain_mesh = 1
    sim = C.c_void_p()
    _abi.check(L.lrl_sim_create(C.byref(env._M), C.byref(P), C.c_int32(5), C.c_int64(0), C.c_uint64(1),
                                C.c_int32(env._dev_index), C.byref(sim)))
    try:
        c = _camera(16, 12, **CHASE)
        L.lrl_set_error(0, b"")
        assert L.lrl_sim_depth(sim, C.byref(c), 0, 5, 0, C.c_void_p(poison.data_ptr()), C.c_void_p(pid.data_ptr()),
                               env._stream()) == -1
        assert b"lrl_sim_set_terrain" in L.lrl_last_error()
    finally:
        L.lrl_sim_destroy(sim)
    torch.cuda.synchronize()
    assert bool((poison == -7).all()) and bool((pid == -7).all())
    assert call() == 0  # and the same call with nothing wrong draws
    torch.cuda.synchronize()
    assert bool((poison > 0).all()) and bool((pid >= 0).all())
