// lrl_depth_sense.hip — the depth sensor model (include/lrl.h: lrl_sim_depth_sense): turns the exact depth image of
// lrl_depth.hip into what a stereo depth camera would deliver: range-dependent noise, holes at depth discontinuities,
// random invalid pixels, a quantised range, and delivery some frames late through a per-env ring.  depth_kernel's
// geometry: one 256-thread workgroup per env, threads walk the image in passes of 256 consecutive pixels, so a wave's
// 64 lanes read and write 64 consecutive floats (256 B) of every array.  The edge test's neighbours are read straight
// from the exact image: read-only, ~12 KB per env, written by the launch before this one.  Every draw is one Philox
// block per (global env id, frame, pixel) on stream LRL_RNG_DEPTH, so the images do not depend on the sharding.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "lrl_kparams.h"
#include "lrl_launch.h"
#include "../../include/lrl_philox.h"

namespace lrl {

namespace {

// the sensed value of a pixel that returned something (z < far) and was not lost: Box-Muller as act_draw's even
// branch (lrl_ppo.hip), sigma = a + b z^2, the range quantised and clamped; every line rounds as written
__device__ __forceinline__ float sense_value(const lrl_depth_sensor& p, float z, float u0, float u1) {
#pragma clang fp contract(off)
  const float g = sqrtf(-2.f * logf(fmaxf(u0, 1e-7f))) * cosf(6.283185307179586f * u1);
  float zn = z + (p.noise_a + p.noise_b * z * z) * g;
  if (p.quant > 0.f) zn = rintf(zn / p.quant) * p.quant;
  return fminf(fmaxf(zn, p.near), p.far);
}

}  // namespace

// depth / sensed: [gridDim.x][H][W]; ring: [gridDim.x][D][H][W], D = latency_max + 1; head / latency: [gridDim.x];
// uniforms (optional): [gridDim.x][H][W][3].  Row b of each belongs to env first_env + b.
__global__ __launch_bounds__(256) void depth_sense_kernel(const uint8_t* __restrict__ reset, int64_t env_offset,
                                                          uint64_t seed, lrl_depth_sensor p, int first_env, int mode,
                                                          uint64_t frame, const float* __restrict__ depth,
                                                          const float* __restrict__ uniforms, float* __restrict__ ring,
                                                          int32_t* __restrict__ head, int32_t* __restrict__ latency,
                                                          float* __restrict__ sensed) {
  const int b = (int)blockIdx.x, env = first_env + b;
  const bool flagged = reset[env] != 0;
  if (mode == LRL_SENSE_RESET_ONLY && !flagged) return;  // (the whole workgroup, before it touches anything)
  const bool fill = mode != LRL_SENSE_PUSH || flagged;
  const int W = p.width, H = p.height, npx = W * H, D = p.latency_max + 1;
  const uint32_t c0 = (uint32_t)(env_offset + env), c1 = (uint32_t)frame;
  const uint32_t c2 = ((uint32_t)LRL_RNG_DEPTH << 16) ^ (uint32_t)(frame >> 32);
  int hd, lat;
  if (fill) {
    // the episode's delay: word 0 of the block at pixel index 0xFFFFFFFF (no pixel has it: W H <= 2^20)
    const int span = p.latency_max - p.latency_min;
    const lrl_u32x4 r = lrl_philox(c0, c1, c2, 0xFFFFFFFFu, seed);
    lat = p.latency_min + min((int)(lrl_u01(r.v[0]) * (float)(span + 1)), span);
    hd = 0;
  } else {
    // (a caller's head and latency are brought into the ring before they index it)
    hd = (int)(((uint32_t)head[b] + 1u) % (uint32_t)D);
    lat = min(max(latency[b], 0), D - 1);
  }
  __syncthreads();  // every thread has read head[b] and latency[b]
  if (threadIdx.x == 0) {
    head[b] = hd;
    latency[b] = lat;
  }
  const float* __restrict__ in = depth + (size_t)b * npx;
  const float* __restrict__ uin = uniforms ? uniforms + (size_t)b * npx * 3 : nullptr;
  float* __restrict__ rg = ring + (size_t)b * D * npx;
  float* __restrict__ out = sensed + (size_t)b * npx;
  const int back = (hd - lat + D) % D;  // the slot delivered by a push (lat < D: never the slot it writes)
#pragma unroll 1
  for (int px = threadIdx.x; px < npx; px += 256) {
    const float z = in[px];
    float v = p.far;
    if (z < p.far) {
      const int i = px / W, j = px - i * W;
      bool lost = false;
      if (p.edge_thresh > 0.f) {
        if (j > 0) { const float zn = in[px - 1]; lost |= fabsf(z - zn) > p.edge_thresh * fminf(z, zn); }
        if (j < W - 1) { const float zn = in[px + 1]; lost |= fabsf(z - zn) > p.edge_thresh * fminf(z, zn); }
        if (i > 0) { const float zn = in[px - W]; lost |= fabsf(z - zn) > p.edge_thresh * fminf(z, zn); }
        if (i < H - 1) { const float zn = in[px + W]; lost |= fabsf(z - zn) > p.edge_thresh * fminf(z, zn); }
      }
      float u0, u1, u2;
      if (uin) {
        u0 = uin[3 * px], u1 = uin[3 * px + 1], u2 = uin[3 * px + 2];
      } else {
        const lrl_u32x4 r = lrl_philox(c0, c1, c2, (uint32_t)px, seed);
        u0 = lrl_u01(r.v[0]), u1 = lrl_u01(r.v[1]), u2 = lrl_u01(r.v[2]);
      }
      lost |= u2 < p.dropout_p;
      v = lost ? p.invalid_value : sense_value(p, z, u0, u1);
    }
    if (fill) {
      for (int d = 0; d < D; ++d) rg[(size_t)d * npx + px] = v;
      out[px] = v;
    } else {
      rg[(size_t)hd * npx + px] = v;
      out[px] = lat ? rg[(size_t)back * npx + px] : v;
    }
  }
}

}  // namespace lrl

extern "C" hipError_t lrl_launch_depth_sense(const KState* S, const lrl_depth_sensor* p, int32_t first_env,
                                             int32_t num_envs, int32_t mode, uint64_t frame, const float* depth,
                                             const float* uniforms, float* ring, int32_t* head, int32_t* latency,
                                             float* sensed, hipStream_t st) {
  if (num_envs < 1) return hipSuccess;
  hipLaunchKernelGGL(lrl::depth_sense_kernel, dim3(num_envs), dim3(256), 0, st, S->reset, S->env_offset, S->seed, *p,
                     first_env, mode, frame, depth, uniforms, ring, head, latency, sensed);
  return hipGetLastError();
}
