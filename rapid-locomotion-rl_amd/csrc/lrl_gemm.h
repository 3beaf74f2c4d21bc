// lrl_gemm.h — LDS-tiled fp32 MFMA GEMM for the PPO minibatch update (gfx950).
//
// C(m, n) = sum_k A(m, k) B(k, n) on v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered FMA chain), with
// the three operand layouts an MLP's forward / backward-data / weight-gradient products need:
//   forward       Y[b][o]  = X[b][i] W[o][i]        A k-contiguous, B k-contiguous   (+bias, ELU)
//   backward-data dX[b][i] = dY[b][o] W[o][i]       A k-contiguous, B n-contiguous   (* ELU'(X))
//   weight grad   dW[o][i] = dY[b][o] X[b][i]       A m-contiguous, B n-contiguous   (split over b)
// The batch dimension of a k-contiguous A (the rows of X) and of an n-contiguous B (the rows of X in
// the weight gradient) may be gathered through an int64 row list — the minibatch indices of
// RolloutStorage.mini_batch_generator (rollout_storage.py:100-137) — so the minibatch is never copied.
//
// The fp32 MFMA kernels behind the launcher (gemm_launch picks by shape; the bf16-split families it tries first —
// x6, x6d, x6p, x6t — are described in lrl_gemm.hip, the dispatch table is DESIGN.md §3).  The (layout, epilogue)
// pairs on offer are NT with EPI_STORE / BIAS / BIAS_ELU / BIAS_TANH, NN with EPI_STORE / DELU / DTANH (and
// EPI_PARTIAL, register-staged only) and TN with EPI_PARTIAL; gemm_launch refuses any other pair before a family is
// tried, and no family instantiates one:
//  * LDS-DMA (NT / NN, every tile interior, float4-aligned operands): 64 x 64 tile, 16-k slices land in a
//    3-stage LDS ring straight from global memory (global_load_lds_dwordx4, counted vmcnt waits, swizzled
//    images read with ds_read_b128), two accumulators per wave;
//  * thin (NT, and NN with EPI_STORE; N <= 32, k = 512 / 1024): op(B) kept in registers per k-quarter, A streamed a
//    block ahead, quarter sums added in wave order;
//  * register-staged (everything else, incl. the split-k weight gradients): a workgroup (4 waves) owns a
//    BM x BN tile (128 / 64 wide, 32 for thin layers); 16-k slices stage through LDS k-major so each MFMA
//    operand is one ds_read_b32 per lane; the next slice is prefetched into registers while the current one
//    is consumed; the tile order is XCD-aware (consecutive tiles on one XCD share the A row block).
// Every path sums k in a fixed order: results are deterministic run to run.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define LRL_GHD __host__ __device__
#else
#define LRL_GHD
#endif

namespace lrl {

enum GemmEpi : int {
  EPI_STORE = 0,     // C = acc
  EPI_BIAS = 1,      // C = acc + bias[n]
  EPI_BIAS_ELU = 2,  // C = elu(acc + bias[n])
  EPI_DELU = 3,      // C = acc * elu'(aux[m][n])  (aux = ELU output of the layer input: elu' = aux > 0 ? 1 : aux + 1)
  EPI_PARTIAL = 4,   // split-k partial: C + split * part_stride (+ bias-gradient partial of A's columns)
  EPI_BIAS_TANH = 5, // C = tanh(acc + bias[n])
  EPI_DTANH = 6,     // C = acc * (1 - aux[m][n]^2)  (aux = tanh output of the layer input)
};

struct GemmP {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* aux;
  const int64_t* a_rows;  // k-contiguous A: row list for m (nullptr = identity)
  const int64_t* b_rows;  // n-contiguous B: row list for k (nullptr = identity)
  float* bias_part;       // EPI_PARTIAL: [splits][groups][M] partial sums over k of A(m, k), or nullptr
  int M, N, K;
  int splits, kps;        // k range of split s: [s*kps, min(K, (s+1)*kps))
  int avec, bvec;         // staging access width (4/2/1 floats), set by gemm_launch from the alignment
  int groups;             // set by gemm_launch
  int64_t lda, ldb, ldc, ld_aux;
  int64_t ga, gb, gc, gbias, gaux;  // per-group element offsets
  int64_t part_stride;              // EPI_PARTIAL: elements between split slices of C ([split][group][M][N])
  // pre-split B (x6p kernel, NT / NN): hi / mid / lo bf16 planes of op(B) in [n][k] form (x6_planes_launch), k padded
  // to bpl_ld (a multiple of 16, zero past K); plane pl of group g at bpl + pl * bpl_ps + g * gbp.  nullptr: B is read
  // as fp32 from `B` by the other kernels
  const uint16_t* bpl;
  int64_t bpl_ld, bpl_ps, gbp;
};

// One weight matrix to split into planes: W is [rows][cols] (ldw) per group (gsrc elements apart); op(B) in [n][k]
// form is W itself (trans = 0: n = row, k = col — the forward's B) or its transpose (trans = 1: n = col, k = row — the
// backward-data B).  dst receives [3][groups][n][kp] bf16 (kp = k rounded up to 16; the padding is zero).
struct PlaneJob {
  const float* W;
  int64_t ldw, gsrc;
  int rows, cols, trans, groups;
  uint16_t* dst;
};
constexpr int MAX_PLANE_JOBS = 8;
LRL_GHD inline int plane_kp(const PlaneJob& j) { return ((j.trans ? j.rows : j.cols) + 15) / 16 * 16; }
LRL_GHD inline int plane_n(const PlaneJob& j) { return j.trans ? j.cols : j.rows; }
LRL_GHD inline int64_t plane_elems(const PlaneJob& j) { return 3ll * j.groups * plane_n(j) * plane_kp(j); }
// Split every job's matrix into its planes (one launch for up to MAX_PLANE_JOBS jobs).
int x6_planes_launch(const PlaneJob* jobs, int n, void* stream);
// false when LRL_GEMM_X6P=0 (no planes: every product reads fp32 B)
bool gemm_x6p_enabled();
// Point p's pre-split B at job j's planes.
inline void gemm_use_planes(GemmP& p, const PlaneJob& j) {
  p.bpl = j.dst;
  p.bpl_ld = plane_kp(j);
  p.gbp = (int64_t)plane_n(j) * plane_kp(j);
  p.bpl_ps = p.gbp * j.groups;
}

// layout: bit0 = A m-contiguous, bit1 = B n-contiguous
enum GemmLayout : int { GEMM_NT = 0, GEMM_NN = 2, GEMM_TN = 3 };

// Enqueue C = op(A, B) for `groups` independent problems of the same shape.  Returns 0 or a negative
// lrl error code (bad shape / unsupported layout).
int gemm_launch(const GemmP& p, int layout, int epi, int groups, void* stream);

// One product of a multi-problem launch: what gemm_launch takes.
struct GemmJob {
  GemmP p;
  int layout, epi, groups;
};
constexpr int MAX_MULTI_JOBS = 3;
// Enqueue 2 or 3 products that do not depend on each other as ONE kernel: its grid is the concatenation of the grids
// gemm_launch would give the jobs, job 0's workgroups first, and every job runs the kernel body, tile and split of its
// own launch, so each output is bit-identical to gemm_launch's.  The job sets on offer are those of the update's backward
// tail, riders first and the large weight gradient (the host) last (lrl_gemm.hip, MultiCombos).  Returns 1 when
// launched, 0 when the set is not one of them (nothing was launched: the caller launches the jobs one by one), or a
// negative lrl error code.  gemm_last_path then reports the last job's family and tile.
int gemm_launch_multi(const GemmJob* jobs, int n, void* stream);

// Kernel family of a launch (the LRL_GEMM_PATH_* values of include/lrl.h)
enum GemmFamily : int {
  FAM_NONE = 0, FAM_X6P = 1, FAM_X6T = 2, FAM_X6 = 3, FAM_X6D = 4, FAM_GLDS = 5, FAM_GLDS32 = 6, FAM_GLDS_TN = 7,
  FAM_THIN16 = 8, FAM_THIN32 = 9, FAM_STAGED = 10,
};
// family | bm << 8 | bn << 16 | interior << 24 (interior: gemm_x6_kernel's unguarded instantiation)
constexpr int gemm_path_id(int family, int bm, int bn, bool interior) {
  return family | (bm << 8) | (bn << 16) | (interior ? 1 << 24 : 0);
}
// The family and tile this thread's last gemm_launch ran on, as a gemm_path_id (0: nothing launched)
int gemm_last_path();

// How a weight-gradient product (reduction over K rows, `groups` problems) is split: the split count.
int gemm_pick_splits(int M, int N, int K, int groups);

// false when the bf16-split families are switched off (LRL_GEMM_X6=0, lrl_debug_gemm_paths): the fp32 MFMA families
// then take every product
bool gemm_x6_enabled();
// the smallest batch (M) of a forward product gemm_x6_kernel takes: below it the product runs on the fp32 MFMA
constexpr int X6_MIN_M = 64;

#ifdef __HIPCC__
// ---- device helpers shared by the x6 GEMM families (lrl_gemm.hip) and the one-launch act (lrl_ppo.hip) ----
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8_t __attribute__((ext_vector_type(8)));
constexpr int XBK = 16;  // k extent of an x6 step and of a plane image's rows

__device__ __forceinline__ float elu_f(float x) { return x > 0.f ? x : expm1f(x); }
// the device library's tanhf: an odd polynomial below |x| = 0.625, so small pre-activations keep their relative
// accuracy (a bare 1 - 2 / (exp(2x) + 1) cancels there: half the digits are gone at |x| = 1e-3), and the function torch
// itself evaluates on the device
__device__ __forceinline__ float tanh_f(float x) { return tanhf(x); }
// epilogue classes: a bias vector added before the activation / the layer input's activation output read as aux
__host__ __device__ constexpr bool epi_bias(int e) { return e == EPI_BIAS || e == EPI_BIAS_ELU || e == EPI_BIAS_TANH; }
__host__ __device__ constexpr bool epi_aux(int e) { return e == EPI_DELU || e == EPI_DTANH; }
// the epilogue's value: v = the accumulator, bj = the column's bias, x = the aux operand (kernels of families without
// an aux epilogue pass 0)
template <int EPI>
__device__ __forceinline__ float epi_apply(float v, float bj, float x) {
  if constexpr (EPI == EPI_BIAS) return v + bj;
  else if constexpr (EPI == EPI_BIAS_ELU) return elu_f(v + bj);
  else if constexpr (EPI == EPI_BIAS_TANH) return tanh_f(v + bj);
  else if constexpr (EPI == EPI_DELU) return x > 0.f ? v : v * (x + 1.f);
  else if constexpr (EPI == EPI_DTANH) return v * (1.f - x * x);
  else return v;
}

__device__ __forceinline__ uint32_t x6_hi_pair(uint32_t u0, uint32_t u1) {
  return __builtin_amdgcn_perm(u1, u0, 0x07060302u);  // (u1 & 0xffff0000) | (u0 >> 16)
}
// (x0, x1) -> the packed bf16 pairs of their hi / mid / lo parts
__device__ __forceinline__ void x6_split2(float x0, float x1, uint32_t& h, uint32_t& m, uint32_t& l) {
  uint32_t u0 = __float_as_uint(x0), u1 = __float_as_uint(x1);
  h = x6_hi_pair(u0, u1);
  float r0 = x0 - __uint_as_float(u0 & 0xffff0000u), r1 = x1 - __uint_as_float(u1 & 0xffff0000u);
  u0 = __float_as_uint(r0);
  u1 = __float_as_uint(r1);
  m = x6_hi_pair(u0, u1);
  r0 = r0 - __uint_as_float(u0 & 0xffff0000u);
  r1 = r1 - __uint_as_float(u1 & 0xffff0000u);
  l = x6_hi_pair(__float_as_uint(r0), __float_as_uint(r1));
}
// bf16 offset of 16-B chunk c of row r in a [R][16] plane image (chunk slots swapped in every other 8-row block: the
// 16-lane groups of a ds_read_b128 operand read stay conflict-free)
__device__ __forceinline__ int x6_off(int r, int c) { return r * XBK + 8 * (c ^ ((r >> 3) & 1)); }

// One 32x32x16 step of the split product: c + a b from the hi / mid / lo planes a[0..2], b[0..2], as the six products
// a2 b0, a1 b1, a0 b2, a1 b0, a0 b1, a0 b0 (smallest first) chained through c.  Every x6 family (x6, x6p, x6t, x6d)
// and the one-launch act take their step from here over the same k order: that one order is what makes their results
// bit-identical.
__device__ __forceinline__ f32x16 x6_mma(const bf16x8_t (&a)[3], const bf16x8_t (&b)[3], f32x16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], c, 0, 0, 0);
  return c;
}
#endif  // __HIPCC__

}  // namespace lrl
