// lrl_raycast.h — the device helpers the two ray casters share (lrl_render.hip: one env per launch from a look-at
// camera; lrl_depth.hip: every env's base-mounted depth camera): the env's primitive list (base box, collision spheres,
// link capsules) rebuilt from the rigid-body state relative to the camera position, the ray / primitive tests, and the
// 2-D DDA over the terrain vertex grid.  Everything sits in an anonymous namespace: each including file gets its own
// copies, inlined into its kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "lrl_kparams.h"

namespace lrl {

namespace {

struct R3 {
  float x, y, z;
};
__device__ __forceinline__ R3 r3(float x, float y, float z) { return R3{x, y, z}; }
__device__ __forceinline__ R3 operator+(R3 a, R3 b) { return r3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ R3 operator-(R3 a, R3 b) { return r3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ R3 operator*(float s, R3 a) { return r3(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ float dot(R3 a, R3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ R3 cross(R3 a, R3 b) {
  return r3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ R3 normalize(R3 a) { return (1.f / sqrtf(dot(a, a))) * a; }

constexpr int NCAP = 3 * LRL_NUM_LEGS;
constexpr float T_NONE = 3.0e38f;

// The env's primitives, camera-relative.  sph: centre, radius (<= 0: none).  cap: end a, unit axis, length, radius
// (<= 0: none).  box: centre, the three axes (rows of the world-from-base rotation's transpose), half extents
// (box[15] <= 0: none).
struct Scene {
  float sph[LRL_MAX_SPHERES][4];
  float cap[NCAP][8];
  float box[16];
  int nsph;
};

// pose of body b of env e: origin and rotation (row-major, from the xyzw quaternion)
__device__ void body_pose(const KState& S, int e, int b, R3& p, float* R) {
  const int N = S.stride;
  const float* rb = S.rb_state + (size_t)b * 13 * N + e;
  p = r3(rb[0], rb[(size_t)N], rb[2 * (size_t)N]);
  const float x = rb[3 * (size_t)N], y = rb[4 * (size_t)N], z = rb[5 * (size_t)N], w = rb[6 * (size_t)N];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
__device__ __forceinline__ R3 rot(const float* R, R3 v) {
  return r3(R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z,
            R[6] * v.x + R[7] * v.y + R[8] * v.z);
}
__device__ R3 sphere_centre(const KParams* __restrict__ K, const KState& S, const KRender& T, int e, int s) {
  R3 p;
  float R[9];
  body_pose(S, e, T.sph_body[s], p, R);
  return p + rot(R, r3(K->sph_pos[s][0], K->sph_pos[s][1], K->sph_pos[s][2]));
}

// thread t builds primitive t: spheres [0, 40), capsules [64, 76), the box 128
__device__ void build_scene(const KParams* __restrict__ K, const KState& S, const KRender& T, int e, R3 cam, int t,
                            Scene& sc) {
  if (t < LRL_MAX_SPHERES) {
    float r = -1.f;
    R3 c = r3(0.f, 0.f, 0.f);
    if (t < K->num_spheres && T.sph_body[t] >= 0 && K->sph_rad[t] > 0.f) {
      c = sphere_centre(K, S, T, e, t) - cam;
      r = K->sph_rad[t];
    }
    sc.sph[t][0] = c.x; sc.sph[t][1] = c.y; sc.sph[t][2] = c.z; sc.sph[t][3] = r;
  } else if (t >= 64 && t < 64 + NCAP) {
    const int i = t - 64;
    float r = -1.f, len = 0.f;
    R3 a = r3(0.f, 0.f, 0.f), u = r3(0.f, 0.f, 1.f);
    const bool has_b = T.cap_b[i] >= 0 || (T.cap_sph[i] >= 0 && T.cap_sph[i] < K->num_spheres && T.sph_body[T.cap_sph[i]] >= 0);
    if (T.cap_a[i] >= 0 && has_b) {
      float R[9];
      R3 b;
      body_pose(S, e, T.cap_a[i], a, R);
      if (T.cap_b[i] >= 0) body_pose(S, e, T.cap_b[i], b, R);
      else b = sphere_centre(K, S, T, e, T.cap_sph[i]);
      const R3 ab = b - a;
      len = sqrtf(dot(ab, ab));
      if (len > 1e-9f) u = (1.f / len) * ab;
      else len = 0.f;
      a = a - cam;
      r = LRL_RENDER_LINK_RADIUS;
    }
    float* c = sc.cap[i];
    c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = u.x; c[4] = u.y; c[5] = u.z; c[6] = len; c[7] = r;
  } else if (t == 128) {
    R3 p;
    float R[9];
    body_pose(S, e, 0, p, R);
    const R3 c = p + rot(R, r3(K->box_c[0], K->box_c[1], K->box_c[2])) - cam;
    sc.box[0] = c.x; sc.box[1] = c.y; sc.box[2] = c.z;
    for (int a = 0; a < 3; ++a)  // axis a of the box in the world frame: column a of R
      for (int k = 0; k < 3; ++k) sc.box[3 + 3 * a + k] = R[3 * k + a];
    sc.box[12] = K->box_h[0]; sc.box[13] = K->box_h[1]; sc.box[14] = K->box_h[2];
    sc.box[15] = (K->box_h[0] > 0.f && K->box_h[1] > 0.f && K->box_h[2] > 0.f) ? 1.f : -1.f;
    sc.nsph = K->num_spheres < LRL_MAX_SPHERES ? K->num_spheres : LRL_MAX_SPHERES;
  }
}

// entry distance of the ray o + t d (|d| = 1) into the sphere (c, r), T_NONE when it misses or starts inside / past
// it: the closest approach first, then the half chord (no difference of two large squares)
__device__ __forceinline__ float ray_sphere(R3 o, R3 d, R3 c, float r) {
  const R3 oc = o - c;
  const float b = dot(oc, d);
  const R3 w = oc - b * d;
  const float disc = r * r - dot(w, w);
  if (!(disc > 0.f)) return T_NONE;
  const float t = -b - sqrtf(disc);
  return t > 0.f ? t : T_NONE;
}

// side of the cylinder around the segment a + y u, y in [0, len]: the same form in the plane across the axis; a ray
// along the axis (no component across it) has no side hit.  The capsule is this plus the two end spheres.
__device__ __forceinline__ float ray_cylinder(R3 o, R3 d, R3 a, R3 u, float len, float r) {
  const R3 oa = o - a;
  const float du = dot(d, u), ou = dot(oa, u);
  const R3 dp = d - du * u, op = oa - ou * u;
  const float A = dot(dp, dp);
  if (!(A > 1e-12f)) return T_NONE;
  const float tc = -dot(dp, op) / A;
  const R3 w = op + tc * dp;
  const float disc = r * r - dot(w, w);
  if (!(disc > 0.f)) return T_NONE;
  const float t = tc - sqrtf(disc / A);
  const float y = ou + t * du;
  return (t > 0.f && y >= 0.f && y <= len) ? t : T_NONE;
}

// slab test against the oriented box; axis = the entry face's axis, sgn the side.  A zero direction component only
// asks whether the origin lies inside that slab (no division).
__device__ __forceinline__ float ray_box(R3 o, R3 d, const float* bx, int& axis, float& sgn) {
  const R3 oc = o - r3(bx[0], bx[1], bx[2]);
  float t0 = -T_NONE, t1 = T_NONE;
  axis = 0;
  sgn = 1.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const R3 ax = r3(bx[3 + 3 * a], bx[4 + 3 * a], bx[5 + 3 * a]);
    const float ol = dot(oc, ax), dl = dot(d, ax), h = bx[12 + a];
    if (fabsf(dl) < 1e-12f) {
      if (fabsf(ol) > h) return T_NONE;
      continue;
    }
    const float inv = 1.f / dl;
    const float ta = (-h - ol) * inv, tb = (h - ol) * inv;
    const float tn = fminf(ta, tb), tf = fmaxf(ta, tb);
    if (tn > t0) { t0 = tn; axis = a; sgn = dl > 0.f ? -1.f : 1.f; }
    t1 = fminf(t1, tf);
  }
  return (t0 <= t1 && t0 > 0.f) ? t0 : T_NONE;
}

// nearest robot primitive along o + t d below tbest: returns its id (0: none), t and the outward normal
__device__ int robot_hit(const Scene& sc, R3 o, R3 d, float& tbest, R3& n) {
  int id = 0, kind = 0, idx = 0, axis = 0;
  float sgn = 1.f;
  if (sc.box[15] > 0.f) {
    int ax;
    float sg;
    const float t = ray_box(o, d, sc.box, ax, sg);
    if (t < tbest) { tbest = t; id = 2; kind = 1; axis = ax; sgn = sg; }
  }
  for (int s = 0; s < sc.nsph; ++s) {
    const float r = sc.sph[s][3];
    if (!(r > 0.f)) continue;
    const float t = ray_sphere(o, d, r3(sc.sph[s][0], sc.sph[s][1], sc.sph[s][2]), r);
    if (t < tbest) { tbest = t; id = 3 + s; kind = 2; idx = s; }
  }
  for (int c = 0; c < NCAP; ++c) {
    const float* q = sc.cap[c];
    const float r = q[7];
    if (!(r > 0.f)) continue;
    const R3 a = r3(q[0], q[1], q[2]), u = r3(q[3], q[4], q[5]);
    float t = ray_cylinder(o, d, a, u, q[6], r);
    t = fminf(t, ray_sphere(o, d, a, r));
    t = fminf(t, ray_sphere(o, d, a + q[6] * u, r));
    if (t < tbest) { tbest = t; id = 3 + LRL_MAX_SPHERES + c; kind = 3; idx = c; }
  }
  if (kind == 1) {
    n = sgn * r3(sc.box[3 + 3 * axis], sc.box[4 + 3 * axis], sc.box[5 + 3 * axis]);
  } else if (kind == 2) {
    n = normalize(o + tbest * d - r3(sc.sph[idx][0], sc.sph[idx][1], sc.sph[idx][2]));
  } else if (kind == 3) {
    const float* q = sc.cap[idx];
    const R3 a = r3(q[0], q[1], q[2]), u = r3(q[3], q[4], q[5]);
    const R3 pa = o + tbest * d - a;
    const float y = fminf(fmaxf(dot(pa, u), 0.f), q[6]);
    n = normalize(pa - y * u);
  }
  return id;
}

__device__ __forceinline__ void clip_axis(float g, float dg, float lo, float hi, float& t0, float& t1) {
  if (fabsf(dg) < 1e-12f) {
    if (g < lo || g > hi) t1 = -1.f;
    return;
  }
  const float inv = 1.f / dg;
  const float ta = (lo - g) * inv, tb = (hi - g) * inv;
  t0 = fmaxf(t0, fminf(ta, tb));
  t1 = fminf(t1, fmaxf(ta, tb));
}

// Möller–Trumbore for a ray from the origin (the vertices are camera-relative); barycentric slack 1e-5 so that a ray
// along a shared edge meets at least one of the two triangles
__device__ __forceinline__ void ray_tri(R3 d, R3 a, R3 b, R3 c, float& tbest, R3& n) {
  const R3 e1 = b - a, e2 = c - a;
  const R3 pv = cross(d, e2);
  const float det = dot(e1, pv);
  if (fabsf(det) < 1e-20f) return;
  const float inv = 1.f / det;
  const R3 tv = r3(-a.x, -a.y, -a.z);
  const float u = dot(tv, pv) * inv;
  const R3 qv = cross(tv, e1);
  const float v = dot(d, qv) * inv;
  const float t = dot(e2, qv) * inv;
  if (u >= -1e-5f && v >= -1e-5f && u + v <= 1.f + 1e-5f && t > 0.f && t < tbest) {
    tbest = t;
    n = cross(e1, e2);
  }
}

// the two triangles of grid cell (i, j) (lrl_sim_set_terrain's: (v(i,j), v(i+1,j+1), v(i,j+1)) and (v(i,j), v(i+1,j),
// v(i+1,j+1))); a cell off the grid has none, and every vertex index is clamped into the grid
__device__ __forceinline__ void cell_tris(const float4* __restrict__ vtx, int R, int C, int i, int j, R3 cam, R3 d,
                                          float& tbest, R3& n) {
  if (i < 0 || i > R - 2 || j < 0 || j > C - 2) return;
  const int i1 = min(i + 1, R - 1), j1 = min(j + 1, C - 1);
  const float4 A = vtx[(size_t)i * C + j], B = vtx[(size_t)i * C + j1], Cc = vtx[(size_t)i1 * C + j],
               D = vtx[(size_t)i1 * C + j1];
  const R3 a = r3(A.x, A.y, A.z) - cam, b = r3(B.x, B.y, B.z) - cam, c = r3(Cc.x, Cc.y, Cc.z) - cam,
           dd = r3(D.x, D.y, D.z) - cam;
  ray_tri(d, a, dd, b, tbest, n);
  ray_tri(d, a, c, dd, tbest, n);
}

// Nearest terrain triangle along cam + t d, t < tbest: a 2-D DDA over the grid cells under the ray.  The trimesh's
// slope correction moves vertices by up to one cell in xy, so a cell's triangles may reach over its neighbours: the
// walk keeps the 3 x 3 cells around the current one tested (the full block at the start, the entering row / column of
// three per step) and goes on until the current cell is entered behind the best hit.  At most
// min(rows + cols, ceil(2 far / horizontal_scale) + 2) steps.
__device__ void terrain_hit(const KParams* __restrict__ K, R3 cam, R3 d, float far, float& tbest, R3& n) {
  const int R = K->terr_rows, C = K->terr_cols;
  const float4* __restrict__ vtx = reinterpret_cast<const float4*>(K->terr_vtx);
  const float bs = K->p.border_size, ih = K->terr_inv_hs;
  const float gx = (cam.x + bs) * ih, gy = (cam.y + bs) * ih, dgx = d.x * ih, dgy = d.y * ih;
  float t0 = 0.f, t1 = fminf(far, tbest);
  clip_axis(gx, dgx, 0.f, (float)(R - 1), t0, t1);
  clip_axis(gy, dgy, 0.f, (float)(C - 1), t0, t1);
  if (!(t0 <= t1)) return;
  const float px = gx + t0 * dgx, py = gy + t0 * dgy;
  int ci = min(max((int)floorf(px), 0), R - 2), cj = min(max((int)floorf(py), 0), C - 2);
  const int si = dgx > 0.f ? 1 : -1, sj = dgy > 0.f ? 1 : -1;
  const bool mx = fabsf(dgx) >= 1e-12f, my = fabsf(dgy) >= 1e-12f;
  const float tdx = mx ? fabsf(1.f / dgx) : T_NONE, tdy = my ? fabsf(1.f / dgy) : T_NONE;
  float tmx = mx ? t0 + (dgx > 0.f ? (float)(ci + 1) - px : px - (float)ci) * tdx : T_NONE;
  float tmy = my ? t0 + (dgy > 0.f ? (float)(cj + 1) - py : py - (float)cj) * tdy : T_NONE;
  for (int a = -1; a <= 1; ++a)
    for (int b = -1; b <= 1; ++b) cell_tris(vtx, R, C, ci + a, cj + b, cam, d, tbest, n);
  const int cap = (int)fminf(ceilf(2.f * far * ih) + 2.f, (float)(R + C));
  for (int step = 0; step < cap; ++step) {
    const bool sx = tmx < tmy;
    const float tenter = sx ? tmx : tmy;  // where the ray enters the next cell
    if (!(tenter <= t1) || tenter > tbest) break;
    if (sx) {
      ci += si;
      tmx += tdx;
      if (ci < 0 || ci > R - 2) break;
      for (int b = -1; b <= 1; ++b) cell_tris(vtx, R, C, ci + si, cj + b, cam, d, tbest, n);
    } else {
      cj += sj;
      tmy += tdy;
      if (cj < 0 || cj > C - 2) break;
      for (int a = -1; a <= 1; ++a) cell_tris(vtx, R, C, ci + a, cj + sj, cam, d, tbest, n);
    }
  }
}

}  // namespace

}  // namespace lrl
