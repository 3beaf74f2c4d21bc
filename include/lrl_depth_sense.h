/* lrl_depth_sense.h - the depth sensor model's part of liblrl's C ABI (include/lrl.h includes this file; lrl_sim,
 * LRL_ABI_VERSION, the LRL_E_* codes and lrl_last_error are declared there).  An appended entry point: no struct or
 * function that existed before changes, so LRL_ABI_VERSION stays. */
#ifndef LRL_DEPTH_SENSE_H_
#define LRL_DEPTH_SENSE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Depth sensor model (project-only, opt-in): what a stereo depth camera would deliver of lrl_sim_depth's exact image —
 * range-dependent noise, holes at depth discontinuities, random invalid pixels, a quantised range, and delivery some
 * frames late.  One launch after the exact image is drawn (csrc/lrl_depth_sense.hip: one 256-thread workgroup per env,
 * passes of 256 consecutive pixels); the exact image is read only.  Appended entry point: LRL_ABI_VERSION stays.
 *   sensed value v of env e (global id g = env_offset + e), call counter `frame`, pixel px = i width + j, exact value
 *   z, in fp32:
 *   1. z >= far: v = far (nothing was hit: no noise, never lost).
 *   2. edge loss, when edge_thresh > 0: the pixel is lost if |z - zn| > edge_thresh min(z, zn) for any of its four
 *      neighbours zn inside the image (a neighbour at `far` counts like any value; the test is symmetric, so both sides
 *      of a discontinuity drop).
 *   3. draws: r = lrl_philox(g, frame's low word, (LRL_RNG_DEPTH << 16) ^ frame's high word, px, seed);
 *      u0, u1, u2 = lrl_u01(r.v[0..2]); or, with `uniforms` (f32 [num_envs][height][width][3]), read from it.
 *   4. dropout: the pixel is lost if u2 < dropout_p.
 *   5. a lost pixel: v = invalid_value.
 *   6. else n = sqrt(-2 ln max(u0, 1e-7)) cos(2 pi u1); zn = z + (noise_a + noise_b z z) n; with quant > 0,
 *      zn = rint(zn / quant) quant; v = min(max(zn, near), far).
 *   latency: env b of the call has a ring[b][D][height][width] with D = latency_max + 1, a head index head[b] and a
 *   delay latency[b] in frames.  A push: head = (head + 1) % D, ring[head] = v, sensed = ring[(head - latency + D) % D].
 *   A fill (a new episode, or the first frame) draws the delay, latency = latency_min + min((int)(lrl_u01(w) *
 *   (latency_max - latency_min + 1)), latency_max - latency_min) with w = word 0 of the same Philox block at pixel
 *   index 0xFFFFFFFF (no pixel has it), then sets head = 0, writes v to all D slots and sensed = v.
 *   cost on an MI355X: DESIGN.md §3.
 * ------------------------------------------------------------------------------------------ */
typedef struct lrl_depth_sensor {
  int32_t width, height;   /* the exact image's */
  float near, far;         /* the exact image's clamps, in metres */
  float noise_a, noise_b;  /* sigma(z) = noise_a + noise_b z^2, metres */
  float dropout_p;         /* share of pixels lost at random */
  float edge_thresh;       /* relative depth step at which both sides drop; 0: no edge loss */
  float invalid_value;     /* what a lost pixel reads */
  float quant;             /* range step in metres; 0: not quantised */
  int32_t latency_min, latency_max; /* the per-episode delay in frames is drawn from [latency_min, latency_max] */
} lrl_depth_sensor;        /* 48 bytes */
/* mode: PUSH pushes every env of the range, an env whose reset flag (LRL_T_RESET) is set fills instead; RESET_ONLY
 * fills the flagged envs and leaves every array of the others untouched; FILL fills every env. */
enum { LRL_SENSE_PUSH = 0, LRL_SENSE_RESET_ONLY = 1, LRL_SENSE_FILL = 2 };
/* One launch on `stream` for envs [first_env, first_env + num_envs); row b of every array belongs to env
 * first_env + b: depth (the exact image, device f32 [num_envs][height][width], read only), uniforms (or NULL), ring
 * (f32 [num_envs][latency_max + 1][height][width]), head and latency (int32 [num_envs]), sensed (f32, depth's shape).
 * Reads the sim's seed, env_offset and reset flags; does not refresh the rigid-body state.  A push brings a head or
 * latency that lies outside the ring into it before use.  LRL_E_INVALID, with a message and no launch: a null sim,
 * sensor, depth, ring, head, latency or sensed; an env range outside the sim; width or height outside [1, 1024];
 * near / far outside 0 <= near < far < 3e38; a negative or non-finite noise_a, noise_b, edge_thresh or quant; dropout_p
 * outside [0, 1]; a non-finite invalid_value; latency_min / latency_max outside 0 <= min <= max <= 15; mode outside
 * 0..2. */
int32_t lrl_sim_depth_sense(lrl_sim* sim, const lrl_depth_sensor* sensor, int32_t first_env, int32_t num_envs,
                            int32_t mode, uint64_t frame, const float* depth, const float* uniforms /* or NULL */,
                            float* ring, int32_t* head, int32_t* latency, float* sensed, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* LRL_DEPTH_SENSE_H_ */
