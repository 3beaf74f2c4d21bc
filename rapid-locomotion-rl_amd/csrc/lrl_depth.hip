// lrl_depth.hip — the egocentric depth camera (include/lrl.h: lrl_sim_depth): one image per env from a camera bolted
// to the env's base, so it rolls, pitches and yaws with the trunk.  One 256-thread workgroup per env: the workgroup
// rebuilds the env's primitive list into LDS once, relative to the camera's position (lrl_raycast.h, as
// lrl_render.hip does), then its threads walk the image in passes of 256 consecutive pixels, so a wave's 64 lanes write
// 64 consecutive floats of the env's [H][W] image.  The value is the planar depth t (d . f), as a depth camera reports
// it, clamped to [near, far]; `far` where nothing is hit within it.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "lrl_kparams.h"
#include "lrl_launch.h"
#include "lrl_raycast.h"

// LRL_DEPTH_CULL (development switch, default on): at scene build, mark a primitive that lies wholly behind the camera
// plane as absent.  Exact: a hit point t d has (t d) . f = t (d . f) > 0 for every ray of the image.
#ifndef LRL_DEPTH_CULL
#define LRL_DEPTH_CULL 1
#endif

namespace lrl {

namespace {

// the primitive thread t built (build_scene's assignment) is dropped when no point of it has x . f > 0
__device__ void cull_behind(Scene& sc, R3 f, int t) {
  if (t < LRL_MAX_SPHERES) {
    const float r = sc.sph[t][3];
    if (r > 0.f && dot(r3(sc.sph[t][0], sc.sph[t][1], sc.sph[t][2]), f) + r <= 0.f) sc.sph[t][3] = -1.f;
  } else if (t >= 64 && t < 64 + NCAP) {
    float* q = sc.cap[t - 64];
    const float r = q[7];
    if (r > 0.f) {
      const R3 a = r3(q[0], q[1], q[2]), u = r3(q[3], q[4], q[5]);
      const float za = dot(a, f), zb = dot(a + q[6] * u, f);
      if (fmaxf(za, zb) + r <= 0.f) q[7] = -1.f;
    }
  } else if (t == 128) {
    if (sc.box[15] > 0.f) {
      float reach = dot(r3(sc.box[0], sc.box[1], sc.box[2]), f);
      for (int a = 0; a < 3; ++a)
        reach += sc.box[12 + a] * fabsf(dot(r3(sc.box[3 + 3 * a], sc.box[4 + 3 * a], sc.box[5 + 3 * a]), f));
      if (reach <= 0.f) sc.box[15] = -1.f;
    }
  }
}

}  // namespace

// depth / ids: [gridDim.x][H][W], image b of env first_env + b
__global__ __launch_bounds__(256) void depth_kernel(const KParams* __restrict__ K, KState S, KRender T,
                                                    lrl_depth_camera cam, int first_env, int only_reset,
                                                    float* __restrict__ depth, int32_t* __restrict__ ids) {
  __shared__ Scene sc;
  const int env = first_env + (int)blockIdx.x;
  if (only_reset && S.reset[env] == 0) return;  // (the whole workgroup, before any barrier)
  const int W = cam.width, H = cam.height, npx = W * H;
  R3 pb;
  float Rb[9];
  body_pose(S, env, 0, pb, Rb);
  const R3 o = pb + rot(Rb, r3(cam.pos[0], cam.pos[1], cam.pos[2]));
  const float pitch = cam.pitch_deg * 0.017453292519943295f;
  const float cp = cosf(pitch), sp = sinf(pitch);
  const R3 f = rot(Rb, r3(cp, 0.f, -sp)), rv = rot(Rb, r3(0.f, -1.f, 0.f)), up = rot(Rb, r3(sp, 0.f, cp));
  const bool robot = !(cam.flags & LRL_DEPTH_NO_ROBOT);
  if (robot) {
    build_scene(K, S, T, env, o, threadIdx.x, sc);
#if LRL_DEPTH_CULL
    cull_behind(sc, f, threadIdx.x);
#endif
    __syncthreads();
  }
  const float th = tanf(0.5f * cam.hfov_deg * 0.017453292519943295f);
  const R3 zero = r3(0.f, 0.f, 0.f);
  const bool mesh = K->p.terrain_mesh != 0;
  float* __restrict__ out = depth + (size_t)blockIdx.x * npx;
  int32_t* __restrict__ out_id = ids ? ids + (size_t)blockIdx.x * npx : nullptr;
#pragma unroll 1
  for (int px = threadIdx.x; px < npx; px += 256) {
    // The scene is loop-invariant, and without this compiler-only fence (no instruction) its ~270 LDS words are
    // hoisted into registers: 256 VGPRs + 15 AGPRs, one wave per SIMD.  With it the primitives are read per pixel, as
    // render_kernel reads them.
    asm volatile("" ::: "memory");
    const int i = px / W, j = px - i * W;
    const float u = (2.f * ((float)j + 0.5f) / (float)W - 1.f) * th;
    const float v = (1.f - 2.f * ((float)i + 0.5f) / (float)H) * th * (float)H / (float)W;
    const R3 d = normalize(f + u * rv + v * up);
    const float tmax = cam.far * sqrtf(1.f + u * u + v * v);  // planar distance `far` along this ray
    float t = tmax;
    R3 n = r3(0.f, 0.f, 1.f);
    int id = robot ? robot_hit(sc, zero, d, t, n) : 0;
    if (mesh) {
      float tg = t;
      terrain_hit(K, o, d, tmax, tg, n);
      if (tg < t) { t = tg; id = 1; }
    } else if (d.z < 0.f && o.z > 0.f) {
      const float tp = -o.z / d.z;
      if (tp < t) { t = tp; id = 1; }
    }
    out[px] = id ? fminf(fmaxf(t * dot(d, f), cam.near), cam.far) : cam.far;
    if (out_id) out_id[px] = id;
  }
}

}  // namespace lrl

extern "C" hipError_t lrl_launch_depth(const KParams* K, const KState* S, const KRender* T, const lrl_depth_camera* cam,
                                       int32_t first_env, int32_t num_envs, int32_t only_reset, float* depth,
                                       int32_t* ids, hipStream_t st) {
  if (num_envs < 1) return hipSuccess;
  hipLaunchKernelGGL(lrl::depth_kernel, dim3(num_envs), dim3(256), 0, st, K, *S, *T, *cam, first_env, only_reset, depth,
                     ids);
  return hipGetLastError();
}
