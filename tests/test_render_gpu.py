"""The headless camera on cuda:0 (lrl_sim_render / lrl_sim_record through LeggedRobotEnv) against the numpy checker
tests/render_ref.py, which tests/test_render_ref.py pins on analytic scenes.

Pass rule of every image comparison (conditions, not measurements): the checker alone, float32 against float64, may
disagree in `ids` on at most 0.25 % of the scene's pixels; the kernel may then disagree with the float64 checker on at
most 0.5 %, and every disagreeing pixel has another id among its 8 neighbours in the checker's image (it sits on a
silhouette or a shadow edge).  On agreeing pixels off every edge (ids and checkerboard cells) colours are within 1 of
255, and depths within DEPTH_REL_BAR of the float64 checker's.

DEPTH_REL_BAR: the worst |d - d64| / d64 measured on an MI355X over the plane scenes of
test_plane_mini_cheetah_images was 2.66e-7 (the 50 x 35 follow image; 1.48e-7, 1.1e-8 and 1.27e-7 on the 16 x 16, 1 x 1
and 33 x 17 images), a few fp32 roundings of metre-sized numbers; the bar is 4 x that, the headroom DESIGN.md §3 gives a
compiler change.
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import render_ref as rr
from lrl import _abi
from lrl import config as lcfg

pytestmark = pytest.mark.gpu

DEPTH_REL_BAR = 4 * 2.66e-7
DEV = "cuda:0"


def _mc_cfg(n, episode_length_s=None):
    cfg = lcfg.make_cfg()
    lcfg.config_mini_cheetah(cfg)
    cfg.env.num_envs = n
    if episode_length_s is not None:
        cfg.env.episode_length_s = episode_length_s
    return cfg


def _model(env):
    M = env._M
    return dict(num_bodies=M.num_bodies, num_spheres=M.num_spheres, body_leg=np.array(M.body_leg[:]),
                body_link=np.array(M.body_link[:]), sphere_body=np.array(M.sphere_body[:]),
                sphere_pos=np.array(M.sphere_pos, np.float32).reshape(_abi.MAX_SPHERES, 3),
                sphere_radius=np.array(M.sphere_radius[:], np.float32))


def _gpu(env, e, cam):
    rgba, dep, ids = env.render_images(e, cam, depth=True, ids=True)
    torch.cuda.synchronize()
    return {"rgba": rgba.cpu().numpy(), "depth": dep.cpu().numpy(), "ids": ids.cpu().numpy()}


def _world_camera(env, e, cam):
    """The camera the kernel forms on the device: the float32 offsets added to env e's float32 base position."""
    pos, tgt = np.array(cam.pos[:], np.float32), np.array(cam.target[:], np.float32)
    if cam.flags & _abi.CAM_FOLLOW:
        base = env.root_states[e, 0:3].cpu().numpy().astype(np.float32)
        pos, tgt = pos + base, tgt + base
    return {"pos": pos.astype(np.float64), "target": tgt.astype(np.float64), "hfov_deg": np.float32(cam.hfov_deg),
            "far": np.float32(cam.far), "width": cam.width, "height": cam.height}


def _compare(env, e, cam, ground_of, label, colour=True, depth=True):
    """Render env e on the GPU and with the checker (from the rigid-body state the render refreshed); apply the pass
    rule.  ground_of(world camera) -> the checker's ground.  Returns the images and the worst relative depth error."""
    k = _gpu(env, e, cam)
    wc = _world_camera(env, e, cam)
    prims = rr.scene_from_state(env.rigid_body_state[e].cpu().numpy(), _model(env))
    ground = ground_of(wc)
    r64 = rr.trace(prims, ground, wc, np.float64)
    r32 = rr.trace(prims, ground, wc, np.float32)
    npx = cam.width * cam.height
    self_bad = int((r32["ids"] != r64["ids"]).sum())
    bad = k["ids"] != r64["ids"]
    edge = rr.boundary(r64["ids"])
    quiet = ~bad & ~rr.boundary(r64["ids"], r64["cell"])
    hit = quiet & (r64["ids"] > 0)
    dcol = int(np.abs(k["rgba"].astype(int) - r64["rgba"].astype(int))[quiet].max()) if quiet.any() else 0
    with np.errstate(invalid="ignore"):
        rel = float((np.abs(k["depth"] - r64["depth"]) / r64["depth"])[hit].max()) if hit.any() else 0.0
    print(f"{label}: {npx} px, checker f32 vs f64 {self_bad}, kernel vs f64 {int(bad.sum())} "
          f"(off an edge {int((bad & ~edge).sum())}), max colour diff {dcol}, max rel depth err {rel:.3e}, "
          f"ids seen {len(np.unique(r64['ids']))}")
    assert self_bad <= 0.0025 * npx, (label, self_bad)
    assert bad.sum() <= 0.005 * npx, (label, int(bad.sum()))
    assert not np.any(bad & ~edge), (label, np.argwhere(bad & ~edge)[:5])
    assert np.all(k["rgba"][..., 3] == 255)
    assert np.all(np.isinf(k["depth"][(k["ids"] == 0)])) and np.all(np.isfinite(k["depth"][k["ids"] != 0]))
    if colour:
        assert dcol <= 1, (label, dcol)
    if depth:
        assert rel < DEPTH_REL_BAR, (label, rel)
    return k, r64, rel


PLANE = lambda wc: ("plane",)


@pytest.fixture(scope="module")
def mc_env():
    from lrl.env import LeggedRobotEnv
    env = LeggedRobotEnv(DEV, cfg=_mc_cfg(5), seed=2)  # 5 envs: the SoA padding to 64 is in play
    env.reset()
    yield env
    env.close()


def test_plane_mini_cheetah_images(mc_env):
    env = mc_env
    assert env.camera_props.width == 360 and env.camera_props.height == 240
    seen = set()
    for e, (w, h) in ((3, (50, 35)), (0, (16, 16)), (4, (1, 1))):
        k, r, _ = _compare(env, e, env._camera(w, h, far=20.0), PLANE, f"plane follow env {e} {w}x{h}")
        seen |= set(r["ids"].ravel().tolist())
    k, r, _ = _compare(env, 2, env._camera(33, 17, offset=(0.0, 0.0, 1.5), far=20.0), PLANE, "plane straight down 33x17")
    seen |= set(r["ids"].ravel().tolist())
    shadows = any(i & rr.SHADOW for i in seen)
    seen = {i & 0xffff for i in seen}
    # the scenes are not empty: sky, ground, the base box, spheres and link capsules were all compared, and shadows
    assert {0, rr.ID_GROUND, rr.ID_BOX} <= seen
    assert any(rr.ID_SPHERE0 <= i < rr.ID_CAPSULE0 for i in seen) and any(i >= rr.ID_CAPSULE0 for i in seen)
    assert shadows
    # env.render(): the reference's (H, W, 4) uint8 image of env 0 from the follow camera
    img = env.render()
    assert img.shape == (240, 360, 4) and img.dtype == np.uint8 and np.all(img[..., 3] == 255)
    np.testing.assert_array_equal(img, _gpu(env, 0, env._camera())["rgba"])


def test_trimesh_go1_image():
    """Go1 on the 3 x 5 borderless tiles of HighLevelControlWrapper.from_actor_critic's env, as a rough trimesh (the Go1
    preset's own ground is the plane, on which that wrapper's tiles are flat and the sim keeps the plane path)."""
    from lrl.env import LeggedRobotEnv
    cfg = lcfg.make_cfg()
    lcfg.config_go1(cfg)
    dr = cfg.domain_rand
    for key in ("push_robots", "randomize_friction", "randomize_restitution", "randomize_motor_strength",
                "randomize_base_mass", "randomize_Kd_factor", "randomize_Kp_factor", "randomize_com_displacement"):
        setattr(dr, key, False)
    cfg.env.num_envs = 3
    t = cfg.terrain
    t.num_rows, t.num_cols, t.border_size = 3, 5, 0
    t.mesh_type, t.curriculum, t.teleport_robots = "trimesh", True, False
    t.terrain_proportions = [0.1, 0.1, 0.35, 0.25, 0.2]  # legged_robot_config.py:57
    t.max_init_terrain_level = min(t.max_init_terrain_level, t.num_rows - 1)
    env = LeggedRobotEnv(DEV, cfg=cfg, seed=3)
    try:
        env.reset()
        assert env._P.terrain_mesh == 1
        t, tc = env.terrain, env.cfg.terrain
        rows, cols = t.heightsamples.shape
        vtx = np.array(t.vertices, np.float32).reshape(rows, cols, 3)
        vtx[..., :2] -= np.float32(tc.border_size)  # (in float32, as lrl_sim_set_terrain places the grid)
        vtx = vtx.astype(np.float64)
        far = 4.0
        ground = lambda wc: ("tris", rr.grid_triangles(vtx, wc["pos"], far + 4 * tc.horizontal_scale))
        k, r, _ = _compare(env, 2, env._camera(48, 32, far=far), ground, "trimesh follow env 2 48x32",
                           colour=False, depth=False)  # (ground-on-ground edges are in no id image)
        kinds = set((r["ids"] & 0xffff).ravel().tolist())
        assert rr.ID_GROUND in kinds and rr.ID_BOX in kinds and len(kinds) > 6
    finally:
        env.close()


def test_after_random_steps(mc_env):
    env = mc_env
    gen = torch.Generator(device=DEV).manual_seed(5)
    for _ in range(10):
        env.step(torch.rand(env.num_envs, 12, device=DEV, generator=gen) * 2 - 1)
    cam = env._camera(50, 35, far=20.0)
    k1, _, _ = _compare(env, 1, cam, PLANE, "plane follow env 1 after 10 random steps", depth=False)
    k0 = _gpu(env, 0, cam)
    assert np.any(k0["rgba"] != k1["rgba"])


def test_refusals_leave_the_outputs_untouched(mc_env):
    env = mc_env
    L, sim, st = _abi.lib(), env._sim, env._stream()
    poison = torch.full((64, 64, 4), 0xAB, dtype=torch.uint8, device=DEV)
    dep = torch.full((64, 64), -7.0, device=DEV)
    ids = torch.full((64, 64), -7, dtype=torch.int32, device=DEV)
    vp = lambda x: C.c_void_p(x.data_ptr())

    def call(e=0, cam=True, rgba=True, **kw):
        c = env._camera(16, 16)
        for key, v in kw.items():
            setattr(c, key, v)
        return L.lrl_sim_render(sim, C.c_int32(e), C.byref(c) if cam else None, vp(poison) if rgba else None, vp(dep),
                                vp(ids), st)
    bad = [dict(e=-1), dict(e=env.num_envs), dict(width=0), dict(width=4097), dict(height=0), dict(height=4097),
           dict(hfov_deg=1.0), dict(hfov_deg=179.0), dict(far=0.0), dict(far=-1.0), dict(cam=False), dict(rgba=False)]
    for kw in bad:
        L.lrl_set_error(0, b"")
        assert call(**kw) == -1, kw
        assert len(L.lrl_last_error()) > 0, kw
    state = torch.zeros(3, dtype=torch.int32, device=DEV)
    c = env._camera(16, 16)
    assert L.lrl_sim_record(sim, C.c_int32(0), C.byref(c), vp(poison), C.c_int32(0), vp(state), st) == -1
    assert L.lrl_sim_record(sim, C.c_int32(0), C.byref(c), vp(poison), C.c_int32(4), None, st) == -1
    assert L.lrl_sim_record(sim, C.c_int32(9), C.byref(c), vp(poison), C.c_int32(4), vp(state), st) == -1
    torch.cuda.synchronize()
    assert bool((poison == 0xAB).all()) and bool((dep == -7.0).all()) and bool((ids == -7).all())
    assert state.tolist() == [0, 0, 0]
    assert call() == 0  # and the same call with nothing wrong draws
    torch.cuda.synchronize()
    assert bool((poison.reshape(-1, 4)[:256, 3] == 255).all()) and bool((poison.reshape(-1, 4)[256:] == 0xAB).all())


def _upstream_env(n, episode_length_s, device_resets=None):
    from lrl.env import LeggedRobotEnv
    env = LeggedRobotEnv(DEV, cfg=_mc_cfg(n, episode_length_s), seed=4, legacy_fork=False, device_resets=device_resets)
    env.reset()
    return env


@pytest.mark.parametrize("device_resets", [True, False])
def test_recording_is_one_full_episode(device_resets):
    env = _upstream_env(4, 0.23, device_resets)  # 12-step episodes: env 0 times out every 13th step
    try:
        assert env._dev_path == device_resets
        act = torch.zeros(4, 12, device=DEV)
        before = torch.cuda.memory_allocated()
        for _ in range(3):  # record_now off: no ring, no state
            env.step(act)
        assert env._rec == {} and env.get_complete_frames() == []
        frame_bytes = 240 * 360 * 4
        assert torch.cuda.memory_allocated() - before < frame_bytes
        env.start_recording()
        assert env._rec["train"]["ring"].shape == (int(env.max_episode_length) + 1, 240, 360, 4)
        shots, resets, got = [], [], []
        for _ in range(45):
            _, _, done, _ = env.step(act)
            shots.append(env.render())
            resets.append(bool(done[0]))
            got = env.get_complete_frames()
            if sum(resets) < 2:
                assert got == []
            else:
                break
        i0, i1 = np.flatnonzero(resets)[:2]
        assert 2 <= i1 - i0 <= int(env.max_episode_length) + 1
        assert len(got) == i1 - i0  # the first reset's step ... the last step before the second reset
        for f, s in zip(got, shots[i0:i1]):
            assert f.shape == (240, 360, 4) and f.dtype == np.uint8
            np.testing.assert_array_equal(f, s)
        assert any(np.any(got[0] != f) for f in got[1:])  # the frames are not one picture
        assert env.get_complete_frames() is got and env.record_now  # kept until pause_recording, as in the reference
        env.pause_recording()
        assert env._rec == {} and not env.record_now and env.get_complete_frames() == []

        # a ring smaller than the episode: the video closes at its capacity (started a few steps before env 0's
        # time-out: with no reset within `capacity` steps the recording would give up instead)
        while int(env.episode_length_buf[0]) < int(env.max_episode_length) - 2:
            env.step(act)
        env.video_capacity = 5
        env.start_recording()
        shots, resets, got = [], [], []
        for _ in range(45):
            _, _, done, _ = env.step(act)
            shots.append(env.render())
            resets.append(bool(done[0]))
            got = env.get_complete_frames()
            if got:
                break
        i0 = int(np.flatnonzero(resets)[0])
        assert len(got) == 5 and len(shots) == i0 + 6 and not any(resets[i0 + 1:])
        for f, s in zip(got, shots[i0:i0 + 5]):
            np.testing.assert_array_equal(f, s)
        env.pause_recording()
    finally:
        env.close()


def test_recording_gives_up_without_a_reset():
    env = _upstream_env(4, None)  # the preset's 20 s episodes: no reset within the ring
    try:
        act = torch.zeros(4, 12, device=DEV)
        env.video_capacity = 4
        env.start_recording()
        for i in range(4):
            assert env.record_now
            env.step(act)
            if i < 3:
                assert env.get_complete_frames() == [] and env.record_now
        assert env.get_complete_frames() == []
        assert not env.record_now and env._rec == {}
    finally:
        env.close()


def test_runner_logs_a_video(tmp_path):
    from lrl.env import LeggedRobotEnv
    from lrl.history import HistoryWrapper
    from lrl.ppo.runner import Logger, Runner, RunnerArgs
    inner = LeggedRobotEnv(DEV, cfg=_mc_cfg(8, 0.23), seed=6, legacy_fork=False)
    env = HistoryWrapper(inner)
    log = []
    step = env.step

    def logged_step(a):
        out = step(a)
        log.append((inner.record_now, bool(out[2][0])))
        return out
    env.step = logged_step
    saved = RunnerArgs.save_video_interval
    RunnerArgs.save_video_interval = 1
    try:
        runner = Runner(env, device=DEV, logger=Logger(str(tmp_path)))
        runner.learn(4)
    finally:
        RunnerArgs.save_video_interval = saved
        inner.close()
    files = sorted(glob.glob(os.path.join(str(tmp_path), "videos", "0000?.npz")))
    assert files, os.listdir(str(tmp_path))
    frames = np.load(files[0])["frames"]
    # env 0's first full episode after recording started: from its first reset to the step before the next
    resets = np.flatnonzero([r and d for r, d in log])
    assert len(resets) >= 2
    T = int(resets[1] - resets[0])
    assert 2 <= T <= int(inner.max_episode_length) + 1
    assert frames.dtype == np.uint8 and frames.shape == (T, 240, 360, 4)
    try:
        import PIL  # noqa: F401
        assert os.path.exists(os.path.splitext(files[0])[0] + ".gif")
    except ImportError:
        pass
