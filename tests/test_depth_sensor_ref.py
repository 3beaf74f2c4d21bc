"""tests/depth_sensor_ref.py (the numpy restatement of the depth sensor model the GPU tests judge the kernel against)
on cases worked out by hand and on the statistics its draws must have."""
import numpy as np

import aux_ref as ar
import depth_sensor_ref as sr
import draws_cases as dc

F32 = np.float32


def _lost(z, thresh, far=3.0):
    p = sr.params(z.shape[1], z.shape[0], far=far, edge_thresh=thresh)
    far_m, edge, drop = sr.masks(z, p, np.ones(z.shape, F32))
    assert not drop.any()
    return far_m, edge


def test_step_edge_drops_both_sides_by_hand():
    z = np.array([[1, 1, 2], [1, 1, 2], [1, 1, 2]], F32)  # |1 - 2| = 1 > 0.1 min(1, 2): columns 1 and 2 are lost
    far, edge = _lost(z, 0.1)
    assert not far.any()
    assert edge.tolist() == [[False, True, True]] * 3
    # exactly at the threshold nothing drops (the test is a strict >), just above it both sides do
    z2 = np.array([[1.0, 1.5, 1.5]], F32)
    assert _lost(z2, 0.5)[1].tolist() == [[False, False, False]]
    assert _lost(z2, 0.4999)[1].tolist() == [[True, True, False]]
    assert _lost(z, 0.0)[1].sum() == 0  # edge_thresh 0: no edge loss
    # a pixel at far is never lost itself, but counts as a neighbour like any value: (0, 0) at far takes (0, 1) and
    # (1, 0) with it; (2, 0) sees only 1s and is the one pixel kept
    z3 = z.copy()
    z3[0, 0] = 3.0
    far, edge = _lost(z3, 0.1)
    assert far.tolist() == [[True, False, False], [False] * 3, [False] * 3]
    assert edge.tolist() == [[False, True, True], [True, True, True], [False, True, True]]
    p = sr.params(3, 3, edge_thresh=0.1, invalid_value=-1.0)
    v = sr.sense(z3, p, np.full((3, 3, 3), 0.5, F32))
    assert v.tolist() == [[3.0, -1.0, -1.0], [-1.0, -1.0, -1.0], [1.0, -1.0, -1.0]]


def test_value_by_hand():
    # u0 = exp(-2) -> rad = 2; u1 = 0 -> n = 2; sigma = 0.01 + 0.02 * 1.5^2 = 0.055; z + sigma n = 1.61
    p = sr.params(1, 1, noise_a=0.01, noise_b=0.02, quant=0.0)
    u = np.array([[[np.exp(-2.0), 0.0, 0.9]]], F32)
    zn, n, rad, sigma = sr.noisy(np.array([[1.5]], F32), p, u)
    assert abs(rad[0, 0] - 2.0) < 1e-6 and abs(n[0, 0] - 2.0) < 1e-6 and abs(sigma[0, 0] - 0.055) < 1e-8
    assert abs(zn[0, 0] - 1.61) < 1e-6
    q = sr.params(1, 1, noise_a=0.01, noise_b=0.02, quant=0.25, near=0.05, far=1.7)
    assert sr.sense(np.array([[1.5]], F32), q, u)[0, 0] == 1.5   # rint(1.61 / 0.25) = 6
    u[0, 0, 1] = 0.5                                              # n = -2: 1.39 -> 1.5 as well (5.56 -> 6)
    assert sr.sense(np.array([[1.5]], F32), q, u)[0, 0] == 1.5
    u[0, 0, 1], u[0, 0, 0] = 0.0, np.exp(-8.0)                    # rad = 4, n = 4: 1.72 -> 1.75 -> clamped to far
    assert sr.sense(np.array([[1.5]], F32), q, u)[0, 0] == float(F32(1.7))
    u[0, 0, 0] = 0.0                                              # the clamp of u0: ln(1e-7), finite
    assert np.isfinite(sr.noisy(np.array([[1.5]], F32), p, u)[0]).all()
    u[0, 0, 2] = 0.0099                                           # dropout at u2 < p
    q.dropout_p = F32(0.01)
    assert sr.sense(np.array([[1.5]], F32), q, u)[0, 0] == float(q.invalid_value)


def _frames(k, h=2, w=3):
    return [np.full((1, h, w), 0.5 + 0.25 * i, F32) for i in range(k)]


def test_zero_model_is_a_pure_delay_line():
    p = sr.params(3, 2, latency=(2, 2))  # no noise, dropout, edge loss or quantisation
    st = sr.state(1, p, dtype=F32)
    imgs = _frames(6)
    got = []
    for t, z in enumerate(imgs):
        v = sr.call(st, p, 9, dc.SEED, sr.FILL if t == 0 else sr.PUSH, [0], t, z, dtype=F32)
        np.testing.assert_array_equal(v, z)
        got.append(st["sensed"].copy())
    assert st["latency"][0] == 2
    for t in range(6):
        np.testing.assert_array_equal(got[t], imgs[max(t - 2, 0)])  # frame t - 2; the fill's before the ring is full
    assert [int((st["ring"][0, d] == imgs[k][0]).all()) for d, k in ((0, 3), (1, 4), (2, 5))] == [1, 1, 1]
    assert st["head"][0] == 5 % 3


def test_fill_rewrites_every_slot_and_modes_pick_their_envs():
    p = sr.params(3, 2, latency=(1, 3))
    n = 4
    st = sr.state(n, p, dtype=F32)
    z = lambda k: np.stack([np.full((2, 3), 0.1 * (b + 1) + k, F32) for b in range(n)])
    sr.call(st, p, 100, dc.SEED, sr.FILL, [0] * n, 0, z(0), dtype=F32)
    assert (st["head"] == 0).all() and ((st["latency"] >= 1) & (st["latency"] <= 3)).all()
    for d in range(4):
        np.testing.assert_array_equal(st["ring"][:, d], z(0))
    np.testing.assert_array_equal(st["sensed"], z(0))
    lat0 = st["latency"].copy()
    # a push with env 2 flagged: env 2 refills (head 0, every slot the new frame, a new delay drawn at this frame)
    sr.call(st, p, 100, dc.SEED, sr.PUSH, [0, 0, 1, 0], 1, z(1), dtype=F32)
    assert st["head"].tolist() == [1, 1, 0, 1]
    for d in range(4):
        np.testing.assert_array_equal(st["ring"][2, d], z(1)[2])
    np.testing.assert_array_equal(st["sensed"][2], z(1)[2])
    np.testing.assert_array_equal(st["sensed"][[0, 1, 3]], z(0)[[0, 1, 3]])  # delay >= 1: still the fill's frame
    assert st["latency"][2] == sr.latency_draw(102, 1, dc.SEED, 1, 3)
    assert (st["latency"][[0, 1, 3]] == lat0[[0, 1, 3]]).all()
    # reset-only with env 1 flagged: env 1 alone changes; with none flagged nothing does
    before = {k: a.copy() for k, a in st.items()}
    sr.call(st, p, 100, dc.SEED, sr.RESET_ONLY, [0, 1, 0, 0], 2, z(2), dtype=F32)
    for k in st:
        np.testing.assert_array_equal(st[k][[0, 2, 3]], before[k][[0, 2, 3]])
    np.testing.assert_array_equal(st["ring"][1], np.broadcast_to(z(2)[1], (4, 2, 3)))
    assert st["head"][1] == 0
    before = {k: a.copy() for k, a in st.items()}
    sr.call(st, p, 100, dc.SEED, sr.RESET_ONLY, [0] * n, 3, z(3), dtype=F32)
    for k in st:
        np.testing.assert_array_equal(st[k], before[k])


def test_latency_draw_stays_in_range_and_covers_it():
    draws = [sr.latency_draw(dc.BIG_OFFSET + e, 3, dc.SEED, 0, 2) for e in range(64)]
    assert set(draws) == {0, 1, 2}
    assert all(sr.latency_draw(e, dc.WRAP, dc.SEED, 4, 4) == 4 for e in range(8))
    assert {sr.latency_draw(e, 7, dc.SEED, 14, 15) for e in range(32)} == {14, 15}
    # the draw is word 0 of the block no pixel uses, on the sensor's own stream, the frame's high word in the key
    c1, c2 = ar.step_key(sr.RNG_DEPTH, dc.WRAP)
    assert (c1, c2) == (0xFFFFFFFF, (8 << 16) ^ 5)
    u = ar.u01(ar.philox(12, c1, c2, 0xFFFFFFFF, dc.SEED)[0])
    assert sr.latency_draw(12, dc.WRAP, dc.SEED, 0, 9) == min(int(F32(u * F32(10))), 9)


def test_pixel_uniforms_are_the_scalar_philox_words():
    u = sr.pixel_uniforms(dc.BIG_OFFSET + 3, dc.WRAP, dc.SEED, 7)
    c1, c2 = ar.step_key(sr.RNG_DEPTH, dc.WRAP)
    for px in (0, 3, 6):
        w = ar.philox((dc.BIG_OFFSET + 3) & ar.M32, c1, c2, px, dc.SEED)
        assert [ar.u01(w[k]) for k in range(3)] == u[px].tolist()
    assert u.dtype == F32 and not np.array_equal(u, sr.pixel_uniforms(dc.BIG_OFFSET + 3, dc.WRAP + 1, dc.SEED, 7))


def test_normals_and_dropout_statistics():
    n = 100_000
    u = sr.pixel_uniforms(17, 2, dc.SEED, n)
    g, _ = ar.box_muller(u[:, 0], u[:, 1], False)
    assert abs(g.mean()) < 5.0 / np.sqrt(n)                # 5 sigma of the mean of n unit normals
    assert abs(g.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)     # ... and of their variance
    for prob in (0.01, 0.2):
        p = sr.params(n, 1, dropout_p=prob)
        far, edge, drop = sr.masks(np.full((1, n), 1.0, F32), p, u[:, 2])
        share = drop.mean()
        assert abs(share - prob) < 5.0 * np.sqrt(prob * (1 - prob) / n), (prob, share)
        assert not far.any() and not edge.any()
    far, edge, drop = sr.masks(np.full((1, n), 3.0, F32), sr.params(n, 1, dropout_p=1.0), u[:, 2])
    assert far.all() and not drop.any()                    # a pixel at far is never lost


def test_share_of_pixels_near_a_quantisation_half_step():
    """With noise and quantisation both on, a kernel within value_bar of the reference may land one step off where the
    reference's unquantised value lies within that bar of a half-step.  The GPU test allows such pixels up to 1 % of an
    image; on its scenes the reference alone has far fewer (about 2e-4 of the kept pixels at quant 0.01)."""
    p = sr.params(40, 30, noise_a=0.002, noise_b=0.01, quant=0.01)
    z = sr.scene(5, 30, 40)
    near_half, kept = 0, 0
    for b in range(5):
        u = sr.pixel_uniforms(dc.BIG_OFFSET + b, 1, dc.SEED, 1200)
        zn, g, rad, sigma = sr.noisy(z[b], p, u)
        bar = sr.value_bar(z[b], g, rad, sigma)
        t = zn / np.float64(p.quant)
        dist = np.abs(t - np.floor(t) - 0.5) * np.float64(p.quant)
        ok = z[b] < p.far
        near_half += int((dist[ok] <= bar[ok] + 2.0 ** -22).sum())  # (+ the division's and product's own roundings)
        kept += int(ok.sum())
    print(f"pixels within the bar of a half-step: {near_half} of {kept}")
    assert kept > 5000 and near_half < 0.01 * kept


def test_scene_has_a_step_a_far_patch_and_smooth_planes():
    for h, w in ((13, 17), (30, 40)):
        z = sr.scene(5, h, w)
        p = sr.params(w, h, edge_thresh=0.1)
        for b in range(5):
            far, edge, _ = sr.masks(z[b], p, np.ones((h, w), F32))
            assert 0 < far.sum() < 0.2 * h * w and 0 < edge.sum() < 0.3 * h * w
            assert (z[b][~far] > 0.5).all() and (z[b][~far] < 2.9).all()
            assert ((~edge) & (~far)).sum() > 0.5 * h * w
