"""tests/depth_ref.py (the numpy checker of the egocentric depth camera) on scenes with closed-form answers, and the
conditions tests/test_depth_gpu.py puts on the checker alone for its terrain scenes (no GPU here)."""
import numpy as np
import pytest

import depth_ref as dr
import depth_scenes as ds
import render_ref as rr


def _cam(**kw):
    cam = dict(pos=(0.0, 0.0, 0.0), pitch_deg=0.0, hfov_deg=87.0, near=0.05, far=3.0, width=33, height=17)
    cam.update(kw)
    return cam


def _uv(cam):
    """The header's image coordinates, restated: u [1, W], v [H, 1]."""
    W, H = cam["width"], cam["height"]
    th = np.tan(np.deg2rad(cam["hfov_deg"]) / 2)
    u = (2 * (np.arange(W) + 0.5) / W - 1) * th
    v = (1 - 2 * (np.arange(H) + 0.5) / H) * th * H / W
    return u[None, :], v[:, None]


def _rot(roll, pitch, yaw):
    """Rz(yaw) Ry(pitch) Rx(roll) from the three elementary matrices (degrees)."""
    r, p, y = np.deg2rad([roll, pitch, yaw])
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _plane_closed_form(cam, R, h):
    """Planar depth of the plane z = 0 from a camera at height h with base rotation R: h / (-d_z) (d . f) per pixel,
    `far` where the ray does not come down or the depth is not below far, clamped below by near."""
    p = np.deg2rad(cam["pitch_deg"])
    f, r, up = R @ [np.cos(p), 0, -np.sin(p)], R @ [0, -1, 0], R @ [np.sin(p), 0, np.cos(p)]
    u, v = _uv(cam)
    d = f[None, None] + u[..., None] * r[None, None] + v[..., None] * up[None, None]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    with np.errstate(divide="ignore"):
        z = np.where(d[..., 2] < 0, h / -d[..., 2] * (d @ f), np.inf)
    hit = z < cam["far"]
    return np.where(hit, np.maximum(z, cam["near"]), np.float64(np.float32(cam["far"]))), hit


IDENT = np.array([0, 0, 0, 1], np.float32)


@pytest.mark.parametrize("pitch", [0.0, 20.0, 60.0])
def test_level_and_pitched_camera_over_the_plane(pitch):
    cam = _cam(pitch_deg=pitch)
    h = 0.31
    got = dr.trace(None, ("plane",), (2.0, -1.0, h), IDENT, cam)
    want, hit = _plane_closed_form(cam, np.eye(3), h)
    np.testing.assert_allclose(got["depth"], want, rtol=1e-12)
    np.testing.assert_array_equal(got["ids"], np.where(hit, rr.ID_GROUND, 0))
    # with the identity base the closed form is simply h / (sin p - v cos p)
    _, v = _uv(cam)
    s = np.sin(np.deg2rad(pitch)) - v * np.cos(np.deg2rad(pitch))
    rows = np.broadcast_to(s, want.shape) > 0
    np.testing.assert_allclose(got["depth"][hit], np.broadcast_to(h / np.where(s > 0, s, 1), want.shape)[hit], rtol=1e-12)
    assert hit.any() and (pitch > 50 or (~hit).any()) and np.all(hit <= rows)


def test_rolled_and_yawed_base():
    cam = _cam(pitch_deg=20.0, pos=(0.27, 0.0, 0.03), width=16, height=16)
    R = _rot(30.0, 0.0, 100.0)
    q = ds.quat_rpy(30.0, 0.0, 100.0).astype(np.float64)
    np.testing.assert_allclose(dr.quat_matrix(q), R, atol=1e-7)  # (the quaternion is rounded to float32)
    R = dr.quat_matrix(q)
    p = np.array([1.0, 2.0, 0.4])
    o = p + R @ cam["pos"]
    got = dr.trace(None, ("plane",), p, q, cam)
    want, hit = _plane_closed_form(cam, R, o[2])
    np.testing.assert_allclose(got["depth"], want, rtol=1e-12)
    np.testing.assert_array_equal(got["ids"] > 0, hit)
    # rolled: the image is not left-right symmetric, as it is without the roll
    assert np.abs(got["depth"] - got["depth"][:, ::-1]).max() > 0.05
    flat = dr.trace(None, ("plane",), p, ds.quat_rpy(0.0, 0.0, 100.0), cam)["depth"]
    np.testing.assert_allclose(flat, flat[:, ::-1], rtol=1e-6)


def test_sphere_on_the_optical_axis():
    cam = _cam(pitch_deg=35.0, width=33, height=17)  # odd sizes: the centre pixel looks along f
    q = ds.quat_rpy(10.0, -20.0, 40.0).astype(np.float64)
    q /= np.linalg.norm(q)  # (rounded to float32 it is not a unit quaternion, and |f| = 1 only to 1e-7)
    p = np.array([0.5, 0.5, 5.0])
    o, f, _, _ = dr.camera_frame(p, q, cam)
    L, rad = 1.25, 0.2
    prims = {"box": None, "spheres": [(4, o + L * f, rad)], "capsules": []}
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-6)):
        got = dr.trace(prims, None, p, q, cam, dtype)
        assert got["ids"][8, 16] == rr.ID_SPHERE0 + 4
        assert abs(got["depth"][8, 16] - (L - rad)) < tol * L
        assert set(np.unique(got["ids"])) == {0, rr.ID_SPHERE0 + 4}
        assert np.all(got["depth"][got["ids"] == 0] == np.float32(cam["far"]))
        # planar depth: every sphere pixel lies between the nearest point and the centre's plane
        z = got["depth"][got["ids"] > 0]
        assert z.min() >= L - rad - tol and z.max() < L


def test_near_and_far_clamping():
    # a camera 3 cm over the plane looking 80 degrees down: every depth is below near = 0.05
    cam = _cam(pitch_deg=80.0, hfov_deg=40.0, width=5, height=5)
    got = dr.trace(None, ("plane",), (0, 0, 0.03), IDENT, cam)
    assert np.all(got["ids"] == rr.ID_GROUND) and np.all(got["depth"] == np.float64(np.float32(0.05)))
    # level camera at 1 m: the plane is within far = 3 only in the lowest rows; the rest is exactly far, id 0
    cam = _cam(width=9, height=9)
    got = dr.trace(None, ("plane",), (0, 0, 1.0), IDENT, cam)
    _, v = _uv(cam)
    want_hit = np.broadcast_to((v < 0) & (1.0 / np.where(v < 0, -v, 1) < 3.0), (9, 9))
    np.testing.assert_array_equal(got["ids"] > 0, want_hit)
    assert want_hit.any() and (~want_hit).any()
    assert np.all(got["depth"][~want_hit] == np.float64(np.float32(3.0)))
    assert np.all(got["depth"][want_hit] < 3.0)
    # far bounds the planar depth, not the ray length: a corner ray is longer than far where its depth is not
    got = dr.trace(None, ("plane",), (0, 0, 1.0), IDENT, _cam(width=9, height=9, far=1.2, pitch_deg=45.0))
    o, f, r, up = dr.camera_frame((0, 0, 1.0), IDENT, _cam(pitch_deg=45.0))
    D, s = dr.rays(_cam(width=9, height=9, pitch_deg=45.0), f, r, up)
    t = 1.0 / -D[:, 2]
    assert np.any((t > 1.2) & (t < 1.2 * np.sqrt(s)) & (got["ids"].ravel() == rr.ID_GROUND))


def test_a_ray_that_starts_inside_the_base_box_does_not_hit_it():
    cam = _cam(pitch_deg=20.0, width=16, height=16)
    p = np.array([0.0, 0.0, 0.4])
    box = (p.copy(), np.eye(3), np.array([0.2, 0.1, 0.05]))  # the camera (pos = 0) sits at its centre
    got = dr.trace({"box": box, "spheres": [], "capsules": []}, ("plane",), p, IDENT, cam)
    assert rr.ID_BOX not in got["ids"]
    np.testing.assert_array_equal(got["depth"], dr.trace(None, ("plane",), p, IDENT, cam)["depth"])
    # moved 30 cm back and up a little, the same box is in view
    cam2 = dict(cam, pos=(-0.5, 0.0, 0.0))
    assert rr.ID_BOX in dr.trace({"box": box, "spheres": [], "capsules": []}, ("plane",), p, IDENT, cam2)["ids"]


@pytest.fixture(scope="module")
def terrain():
    cfg = ds.go1_trimesh_cfg()
    return cfg, ds.terrain_vertices(cfg)


@pytest.mark.parametrize("e", sorted(ds.TERRAIN_SCENES))
def test_terrain_scenes_meet_the_gpu_tests_conditions_on_the_checker(terrain, e):
    """What test_depth_gpu.py's terrain test asks of the reference alone: float32 and float64 ids disagree on at most
    0.25 % of the pixels, and at least three quarters of the ground pixels are quiet (depth_ref.quiet_ground)."""
    cfg, vtx = terrain
    sc = ds.TERRAIN_SCENES[e]
    cam = ds.terrain_camera(sc["cam"])
    pos, q = np.float32(sc["pos"]), ds.quat_rpy(*sc["rpy"])
    # (every triangle a ray can reach: rays end at planar distance far, so a corner ray is longer than far)
    ground = ("tris", rr.grid_triangles(vtx, pos, ds.reach(cam) + 4 * cfg.terrain.horizontal_scale))
    r64, quiet = dr.quiet_ground(ground, pos, q, cam)
    r32 = dr.trace(None, ground, pos, q, cam, np.float32)
    npx = cam["width"] * cam["height"]
    g = r64["ids"] == rr.ID_GROUND
    print(f"terrain scene {e}: ground {int(g.sum())} of {npx} px, quiet {int(quiet.sum())}, "
          f"f32 vs f64 ids {int((r32['ids'] != r64['ids']).sum())}")
    assert (r32["ids"] != r64["ids"]).sum() <= 0.0025 * npx
    assert g.sum() > 0 and quiet.sum() >= 0.75 * g.sum()
    assert np.all(r64["depth"][~g] == np.float64(np.float32(cam["far"])))
    if e == 0:  # looking out over the grid's edge: rays leave the grid
        assert (~g).sum() > 0.25 * npx
    if e == 1:  # far = 0.5: most pixels see nothing within it
        assert (~g).sum() > 0.5 * npx
