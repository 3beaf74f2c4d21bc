"""The numpy checker of the camera (tests/render_ref.py) on scenes with analytic answers, so that the GPU tests'
kernel-vs-checker comparison is not circular; and its float32 form against its float64 form at the image sizes the GPU
tests use (the id disagreements a float32 tracer of these definitions may have, half the GPU tests' own cap)."""
import numpy as np
import pytest

import render_ref as rr
from lrl import _abi

LIGHT = rr._unit(rr._c(_abi.RENDER_LIGHT))
AMB = float(rr._c(_abi.RENDER_AMBIENT))


def _cam(pos, target, w, h, hfov=90.0, far=100.0):
    return {"pos": pos, "target": target, "hfov_deg": hfov, "far": far, "width": w, "height": h}


def _shade(albedo, n, lit=True):
    k = AMB + (1 - AMB) * max(0.0, float(np.dot(n, LIGHT))) * (1.0 if lit else 0.0)
    return np.floor(255 * np.clip(rr._c(albedo) * k, 0, 1) + 0.5).astype(np.uint8)


def test_sphere_depth_and_silhouette():
    d, r, W = 3.0, 0.4, 65
    out = rr.trace({"spheres": [(5, [d, 0, 0], r)]}, None, _cam([0, 0, 0], [1, 0, 0], W, W))
    c = W // 2
    assert out["depth"][c, c] == pytest.approx(d - r, rel=1e-14)
    # (the face towards the camera looks away from the light: its shadow ray goes through the sphere itself)
    assert out["ids"][c, c] == (rr.ID_SPHERE0 + 5) | rr.SHADOW
    np.testing.assert_array_equal(out["rgba"][c, c], list(_shade(_abi.RENDER_SPHERE, [-1, 0, 0])) + [255])
    # a pixel of the centre row sees the sphere iff the tangent of its angle off the axis is below r / sqrt(d^2 - r^2)
    u = 2 * (np.arange(W) + 0.5) / W - 1
    np.testing.assert_array_equal(out["ids"][c] != 0, np.abs(u) < r / np.sqrt(d * d - r * r))
    np.testing.assert_array_equal(out["ids"][:, c] != 0, np.abs(u) < r / np.sqrt(d * d - r * r))
    assert np.all(np.isinf(out["depth"][out["ids"] == 0]))
    assert tuple(out["rgba"][0, 0]) == tuple(np.floor(255 * rr._c(_abi.RENDER_SKY) + 0.5).astype(int)) + (255,)


def test_axis_aligned_box_faces():
    h = np.array([0.3, 0.2, 0.1])
    box = {"box": ([0, 0, 0], np.eye(3), h)}
    for pos, n, dist in (([2, 0, 0], [1, 0, 0], 2 - 0.3), ([0, -2, 0], [0, -1, 0], 2 - 0.2),
                         ([0, 1e-9, 2], [0, 0, 1], 2 - 0.1)):
        out = rr.trace(box, None, _cam(pos, [0, 0, 0], 33, 33))
        assert out["ids"][16, 16] == rr.ID_BOX
        assert out["depth"][16, 16] == pytest.approx(dist, rel=1e-9)
        np.testing.assert_array_equal(out["rgba"][16, 16, :3], _shade(_abi.RENDER_BASE, n))
    # a ray with zero components (along -x exactly) gives no NaN anywhere
    out = rr.trace(box, None, _cam([2, 0, 0], [0, 0, 0], 33, 33))
    assert not np.any(np.isnan(out["depth"]))


def test_rotated_box_faces():
    a = np.pi / 4
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    out = rr.trace({"box": ([0, 0, 0], R, [0.2, 0.2, 0.5])}, None, _cam([3, 0, 0], [0, 0, 0], 65, 65, hfov=30.0))
    # the camera looks at the vertical edge at x = 0.2 sqrt(2); the faces either side are box +x (normal R[:, 0], towards
    # +y in the world, image left: r = f x z = +y for f = -x) and box -y (normal -R[:, 1])
    assert out["depth"][32, 32] == pytest.approx(3 - 0.2 * np.sqrt(2), rel=1e-3)
    np.testing.assert_array_equal(out["rgba"][32, 36, :3], _shade(_abi.RENDER_BASE, R[:, 0]))
    np.testing.assert_array_equal(out["rgba"][32, 28, :3], _shade(_abi.RENDER_BASE, -R[:, 1]))
    # depth on the +x face along the centre row: the plane n . p = 0.2
    n = R[:, 0]
    d = rr.camera_rays(_cam([3, 0, 0], [0, 0, 0], 65, 65, hfov=30.0)).reshape(65, 65, 3)[32, 36]
    assert out["depth"][32, 36] == pytest.approx((0.2 - n @ np.array([3.0, 0, 0])) / (n @ d), rel=1e-12)


def test_capsule_end_on_and_side_on():
    cam = _cam([0, 0, 0], [1, 0, 0], 65, 65)
    end = rr.trace({"capsules": [(7, [2, 0, 0], [3, 0, 0], 0.1)]}, None, cam)
    assert end["depth"][32, 32] == pytest.approx(1.9, rel=1e-14)
    assert end["ids"][32, 32] & 0xffff == rr.ID_CAPSULE0 + 7
    side = rr.trace({"capsules": [(0, [2, -0.5, 0], [2, 0.5, 0], 0.1)]}, None, cam)
    assert side["depth"][32, 32] == pytest.approx(1.9, rel=1e-14)
    # centre row, a column looking at y = 2 u inside the straight part: the ray (1, u, 0) / |.| meets the cylinder
    # about the line x = 2, z = 0 where its x reaches 1.9
    D = rr.camera_rays(cam).reshape(65, 65, 3)
    for j in (26, 30, 38):
        assert abs(2 * D[32, j, 1] / D[32, j, 0]) < 0.45
        assert side["depth"][32, j] == pytest.approx(1.9 / D[32, j, 0], rel=1e-12)
    # and past the end sphere nothing: |y| > 0.6 at x = 2
    assert side["ids"][32, 0] == 0 and side["ids"][32, 64] == 0
    # past the straight part the end sphere is seen: the hit point lies on the sphere about b
    j = int(np.argmin(np.abs(2 * D[32, :, 1] / D[32, :, 0] - 0.58)))
    p = side["depth"][32, j] * D[32, j]
    assert side["ids"][32, j] != 0 and p[1] > 0.5
    assert np.linalg.norm(p - [2, 0.5, 0]) == pytest.approx(0.1, rel=1e-12)


def test_plane_horizon_row():
    H, W, alpha, hgt = 40, 30, np.deg2rad(20.0), 1.5
    cam = _cam([0, 0, hgt], [np.cos(alpha), 0, hgt - np.sin(alpha)], W, H, far=1e6)
    out = rr.trace({}, ("plane",), cam)
    v = (1 - 2 * (np.arange(H) + 0.5) / H) * H / W
    # at u ~ 0: d.z ~ -sin(alpha) + v cos(alpha); the ground shows where v < tan(alpha)
    np.testing.assert_array_equal(out["ids"][:, W // 2] != 0, v < np.tan(alpha))
    i = H - 1
    D = rr.camera_rays(cam).reshape(H, W, 3)
    assert out["depth"][i, 3] == pytest.approx(hgt / -D[i, 3, 2], rel=1e-14)
    # far cuts the plane off
    near = rr.trace({}, ("plane",), dict(cam, far=3.0))
    np.testing.assert_array_equal(near["ids"] != 0, out["depth"] < 3.0)
    # checkerboard: the hit point's cell decides the colour
    p = np.array([0, 0, hgt]) + out["depth"][i, 3] * D[i, 3]
    par = (int(np.floor(p[0])) + int(np.floor(p[1]))) & 1
    np.testing.assert_array_equal(out["rgba"][i, 3, :3],
                                  _shade(_abi.RENDER_GROUND_B if par else _abi.RENDER_GROUND_A, [0, 0, 1]))
    assert out["cell"][i, 3] == 1 + par


def test_ramp_grid_matches_analytic_plane():
    xs, ys = np.arange(-2, 1.51, 0.25), np.arange(-1, 1.01, 0.25)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    a, b, c = 0.3, -0.1, 0.2
    vtx = np.stack([X, Y, a * X + b * Y + c], -1)
    pos = np.array([-1.0, 0.2, 2.0])
    cam = _cam(pos, [0.5, 0.0, 0.0], 31, 21, hfov=60.0, far=50.0)
    out = rr.trace({}, ("tris", rr.grid_triangles(vtx, pos, 50.0)), cam)
    D = rr.camera_rays(cam).reshape(21, 31, 3)
    n = np.array([-a, -b, 1.0])
    t = (c - n @ pos) / (D @ n)
    p = pos + t[..., None] * D
    inside = (t > 0) & (p[..., 0] > xs[0]) & (p[..., 0] < xs[-1]) & (p[..., 1] > ys[0]) & (p[..., 1] < ys[-1])
    assert inside.sum() > 100 and (~inside).sum() > 100  # outside the grid there is no ground
    np.testing.assert_array_equal(out["ids"] == rr.ID_GROUND, inside)
    np.testing.assert_allclose(out["depth"][inside], t[inside], rtol=1e-12)
    lit = _shade(_abi.RENDER_GROUND_A, n / np.linalg.norm(n))
    assert np.any(np.all(out["rgba"][..., :3] == lit, axis=-1))


def test_straight_down_camera_uses_the_y_fallback():
    f, r, up = rr.camera_basis([0, 0, 2], [0, 0, 0])
    np.testing.assert_allclose(f, [0, 0, -1])
    np.testing.assert_allclose(r, [1, 0, 0], atol=1e-15)   # f x y
    np.testing.assert_allclose(up, [0, 1, 0], atol=1e-15)
    cam = _cam([0, 0, 2], [0, 0, 0], 33, 33)
    out = rr.trace({"spheres": [(0, [0.5, 0, 0.1], 0.1), (1, [0, 1.0, 0.1], 0.1)]}, ("plane",), cam)
    assert out["depth"][16, 16] == pytest.approx(2.0)
    i0, j0 = np.argwhere((out["ids"] & 0xffff) == rr.ID_SPHERE0).mean(0)
    i1, j1 = np.argwhere((out["ids"] & 0xffff) == rr.ID_SPHERE0 + 1).mean(0)
    assert j0 > 18 and abs(i0 - 16) < 1      # +x is image right
    assert i1 < 10 and abs(j1 - 16) < 1      # +y is image up
    # the spheres' shadows fall on the plane away from the light (light from +x, -y: shadows towards -x, +y)
    sh = np.argwhere(out["ids"] == (rr.ID_GROUND | rr.SHADOW))
    assert len(sh) > 0


def robot_like_scene(origin=(0.0, 0.0, 0.0)):
    """A quadruped-shaped set of primitives (box, hip / knee / foot spheres, three capsules per leg) standing on z = 0."""
    o = np.asarray(origin, np.float64)
    prims = {"box": (o + [0, 0, 0.32], rr.quat_to_matrix([0.02, -0.03, 0.05, 0.998]), [0.19, 0.05, 0.045]),
             "spheres": [], "capsules": []}
    s = 8
    for leg, (sx, sy) in enumerate(((1, 1), (1, -1), (-1, 1), (-1, -1))):
        hip = o + [0.19 * sx, 0.05 * sy, 0.32]
        thigh = hip + [0, 0.06 * sy, 0]
        knee = thigh + [-0.12, 0.01 * sy, -0.17]
        foot = knee + [0.10, 0, -0.13 + 0.02]
        prims["spheres"] += [(s, hip, 0.045), (s + 1, knee, 0.03), (s + 2, foot, 0.02)]
        s += 3
        prims["capsules"] += [(3 * leg, hip, thigh, 0.02), (3 * leg + 1, thigh, knee, 0.02),
                              (3 * leg + 2, knee, foot, 0.02)]
    return prims


GPU_TEST_SIZES = [(50, 35), (16, 16), (1, 1), (33, 17), (48, 32)]


@pytest.mark.parametrize("w,h", GPU_TEST_SIZES)
def test_float32_checker_agrees_with_float64(w, h):
    origin = np.array([12.3, -7.9, 0.0])
    prims = robot_like_scene(origin)
    base = origin + [0, 0, 0.32]
    seen = set()
    for pos in (base + [0, -1, 1], base + [0, 0, 1.2]):
        cam = _cam(pos, base, w, h, far=20.0)
        a = rr.trace(prims, ("plane",), cam, np.float64)
        b = rr.trace(prims, ("plane",), cam, np.float32)
        bad = a["ids"] != b["ids"]
        assert bad.sum() <= 0.00125 * w * h, (int(bad.sum()), w * h)  # half the GPU tests' 0.25 % cap
        assert not np.any(bad & ~rr.boundary(a["ids"]))
        seen |= set(np.unique(a["ids"]).tolist())
    if w >= 33:  # box, spheres, capsules, ground and shadows are all in view
        kinds = np.array(sorted(seen)) & 0xffff
        assert rr.ID_GROUND in kinds and rr.ID_BOX in kinds and any(k & rr.SHADOW for k in seen)
        assert np.any((kinds >= rr.ID_SPHERE0) & (kinds < rr.ID_CAPSULE0)) and np.any(kinds >= rr.ID_CAPSULE0)
