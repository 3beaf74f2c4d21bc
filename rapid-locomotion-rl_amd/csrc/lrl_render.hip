// lrl_render.hip — the headless camera (include/lrl.h: lrl_sim_render / lrl_sim_record): a ray caster over one env's
// collision model.  One thread per pixel, 256-thread workgroups on 16 x 16 pixel tiles; every workgroup rebuilds the
// env's primitive list (base box, collision spheres, link capsules) from the rigid-body state into LDS, relative to the
// camera position (differences of nearby fp32 world coordinates lose nothing; distances along the ray then carry the
// rounding of ~1 m numbers whatever the env's distance from the world origin).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "lrl_kparams.h"
#include "lrl_launch.h"
#include "lrl_raycast.h"

namespace lrl {

namespace {

__device__ __forceinline__ uint32_t to_byte(float c) {
  return (uint32_t)floorf(255.f * fminf(fmaxf(c, 0.f), 1.f) + 0.5f);
}

}  // namespace

// slot: null (lrl_sim_render), or lrl_sim_record's state word 2: the ring slot of this frame, < 0 = no frame
__global__ __launch_bounds__(256) void render_kernel(const KParams* __restrict__ K, KState S, KRender T, lrl_camera cam,
                                                     int env, uint8_t* __restrict__ rgba, float* __restrict__ depth,
                                                     int32_t* __restrict__ ids, const int32_t* __restrict__ slot) {
  __shared__ Scene sc;
  const int W = cam.width, H = cam.height;
  if (slot) {
    const int sl = *slot;
    if (sl < 0) return;
    rgba += (size_t)sl * W * H * 4;
  }
  const int N = S.stride;
  R3 o = r3(cam.pos[0], cam.pos[1], cam.pos[2]), tg = r3(cam.target[0], cam.target[1], cam.target[2]);
  if (cam.flags & LRL_CAM_FOLLOW) {
    const R3 base = r3(S.root[env], S.root[N + env], S.root[2 * N + env]);
    o = o + base;
    tg = tg + base;
  }
  build_scene(K, S, T, env, o, threadIdx.x, sc);
  __syncthreads();
  const int j = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= H || j >= W) return;
  const R3 f = normalize(tg - o);
  R3 rv = cross(f, r3(0.f, 0.f, 1.f));
  if (sqrtf(dot(rv, rv)) < 1e-6f) rv = cross(f, r3(0.f, 1.f, 0.f));
  rv = normalize(rv);
  const R3 up = cross(rv, f);
  const float th = tanf(0.5f * cam.hfov_deg * 0.017453292519943295f);
  const float u = (2.f * ((float)j + 0.5f) / (float)W - 1.f) * th;
  const float v = (1.f - 2.f * ((float)i + 0.5f) / (float)H) * th * (float)H / (float)W;
  const R3 d = normalize(f + u * rv + v * up);
  const R3 zero = r3(0.f, 0.f, 0.f);

  float t = cam.far;
  R3 n = r3(0.f, 0.f, 1.f);
  int id = robot_hit(sc, zero, d, t, n);
  if (K->p.terrain_mesh) {
    float tg2 = t;
    R3 ng = n;
    terrain_hit(K, o, d, cam.far, tg2, ng);
    if (tg2 < t) {
      t = tg2;
      id = 1;
      ng = normalize(ng);
      n = dot(ng, d) > 0.f ? r3(-ng.x, -ng.y, -ng.z) : ng;
    }
  } else if (d.z < 0.f && o.z > 0.f) {
    const float tp = -o.z / d.z;
    if (tp < t) { t = tp; id = 1; n = r3(0.f, 0.f, 1.f); }
  }

  R3 col = r3(LRL_RENDER_SKY_R, LRL_RENDER_SKY_G, LRL_RENDER_SKY_B);
  if (id) {
    const R3 p = t * d;
    R3 alb;
    if (id == 1) {
      const int cell = (int)floorf(o.x + p.x) + (int)floorf(o.y + p.y);
      alb = (cell & 1) ? r3(LRL_RENDER_GROUND_B_R, LRL_RENDER_GROUND_B_G, LRL_RENDER_GROUND_B_B)
                       : r3(LRL_RENDER_GROUND_A_R, LRL_RENDER_GROUND_A_G, LRL_RENDER_GROUND_A_B);
    } else if (id == 2) {
      alb = r3(LRL_RENDER_BASE_R, LRL_RENDER_BASE_G, LRL_RENDER_BASE_B);
    } else if (id < 3 + LRL_MAX_SPHERES) {
      alb = r3(LRL_RENDER_SPHERE_R, LRL_RENDER_SPHERE_G, LRL_RENDER_SPHERE_B);
    } else {
      alb = r3(LRL_RENDER_LINK_R, LRL_RENDER_LINK_G, LRL_RENDER_LINK_B);
    }
    const R3 l = normalize(r3(LRL_RENDER_LIGHT_X, LRL_RENDER_LIGHT_Y, LRL_RENDER_LIGHT_Z));
    float ts = T_NONE;
    R3 ns;
    const bool shadow = robot_hit(sc, p + 1e-3f * n, l, ts, ns) != 0;
    if (shadow) id |= LRL_RENDER_ID_SHADOW;
    const float k = LRL_RENDER_AMBIENT + (1.f - LRL_RENDER_AMBIENT) * fmaxf(0.f, dot(n, l)) * (shadow ? 0.f : 1.f);
    col = k * alb;
  }
  const size_t px = (size_t)i * W + j;
  reinterpret_cast<uchar4*>(rgba)[px] = make_uchar4((unsigned char)to_byte(col.x), (unsigned char)to_byte(col.y),
                                                    (unsigned char)to_byte(col.z), 255);
  if (depth) depth[px] = id ? t : INFINITY;
  if (ids) ids[px] = id;
}

// lrl_sim_record's state machine (include/lrl.h): st = (phase, count, slot)
__global__ void record_state_kernel(KState S, int env, int capacity, int32_t* __restrict__ st) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int phase = st[0], count = st[1];
  const bool reset = S.reset[env] != 0;
  if (phase == 0) {
    if (reset) { phase = 1; count = 0; }
    else if (++count >= capacity) phase = 3;
  } else if (phase == 1 && (reset || count >= capacity)) {
    phase = 2;
  }
  st[2] = phase == 1 ? count++ : -1;
  st[0] = phase;
  st[1] = count;
}

}  // namespace lrl

extern "C" hipError_t lrl_launch_render(const KParams* K, const KState* S, const KRender* T, const lrl_camera* cam,
                                        int32_t env, uint8_t* rgba, float* depth, int32_t* ids, const int32_t* slot,
                                        hipStream_t st) {
  const dim3 grid((cam->width + 15) / 16, (cam->height + 15) / 16);
  hipLaunchKernelGGL(lrl::render_kernel, grid, dim3(256), 0, st, K, *S, *T, *cam, env, rgba, depth, ids, slot);
  return hipGetLastError();
}

extern "C" hipError_t lrl_launch_record_state(const KState* S, int32_t env, int32_t capacity, int32_t* state,
                                              hipStream_t st) {
  hipLaunchKernelGGL(lrl::record_state_kernel, dim3(1), dim3(64), 0, st, *S, env, capacity, state);
  return hipGetLastError();
}
