// lrl_ppo.hip — PPO.update (mini_gym_learn/ppo/ppo.py:94-178) for gfx950.
//
// Per minibatch (B rows gathered through the randperm slice, never copied):
//   phase 1  lrl_ppo_forward_backward      encoder / actor / critic forward (grouped fp32-MFMA GEMMs,
//            bias+ELU fused), one "head" kernel for the distribution, losses (clipped surrogate,
//            clipped value loss, entropy), KL and the loss gradient, then the backward pass
//            (backward-data GEMMs with ELU' fused, split-k weight-gradient GEMMs) and one segmented
//            reduction that lands every gradient in the flat grad buffer;
//   phase 2  lrl_ppo_optimizer_step        adaptive-KL learning rate, clip_grad_norm_, Adam — all on the
//            device (the learning rate lives in lrl_ppo_ctrl), so a single-GPU update never syncs the host;
//   phase 3  lrl_ppo_adaptation_forward_backward   target = encoder(priv) with the updated weights,
//            adaptation_module(history) forward, MSE and backward;
//   phase 4  lrl_ppo_adaptation_step       Adam on the adaptation module (Q14: the second optimiser only
//            ever sees adaptation-module gradients).
// Between phases 1/2 and 3/4 a multi-GPU caller all-reduces grads[main_begin:kl_slot+1) /
// grads[adapt_begin:adapt_end) (one flat RCCL all-reduce each) and passes grad_scale = 1/world.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <vector>

#include "../../include/lrl.h"
#include "../../include/lrl_philox.h"
#include "lrl_gemm.h"
#include "lrl_launch.h"

namespace lrl {

constexpr float LOG_SQRT_2PI = 0.91893853320467274178f;  // math.log(math.sqrt(2 * math.pi))
constexpr int HEAD_ROWS = 32;                             // rows per head workgroup (LDS ~45 KB: 3 per CU)
constexpr int HEAD_THREADS = 256;
constexpr int HEAD_W = 128;                               // actor / critic last hidden width (ac_h2)
constexpr int MAX_ACT = 16;
constexpr int HEAD_NA = 12;  // the PPO head kernel is specialised for the quadrupeds' 12 actions
constexpr int MAX_LAT = 32;

__device__ __forceinline__ float delu(float h) { return h > 0.f ? 1.f : h + 1.f; }  // elu'(y) from h = elu(y)

// ---------------------------------------------------------------------------------------------------
// gather obs rows into the actor/critic input X = [obs | latent | 0-pad] ([B][64])
// thread = (group of PREP_R rows, column): the group's row indices, then its values, are loaded before any store, so
// a thread has PREP_R gathers in flight and the grid is resident in one round (one thread per element left most of
// a minibatch's workgroups waiting behind two dependent load latencies)
constexpr int PREP_R = 4;
__global__ void ppo_prep_kernel(const float* __restrict__ obs, const int64_t* __restrict__ rows, int B, int no,
                                int xs, float* __restrict__ X) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t ng = ((int64_t)B + PREP_R - 1) / PREP_R;
  if (i >= ng * xs) return;
  const int g = (int)(i / xs), c = (int)(i - (int64_t)g * xs);
  int64_t src[PREP_R];
  float v[PREP_R];
#pragma unroll
  for (int u = 0; u < PREP_R; ++u) {
    const int b = g * PREP_R + u;
    src[u] = b < B ? (rows ? rows[b] : (int64_t)b) : -1;
  }
#pragma unroll
  for (int u = 0; u < PREP_R; ++u) v[u] = (c < no && src[u] >= 0) ? obs[src[u] * no + c] : 0.f;
#pragma unroll
  for (int u = 0; u < PREP_R; ++u) {
    const int b = g * PREP_R + u;
    if (b < B) X[(int64_t)b * xs + c] = v[u];
  }
}

inline unsigned prep_blocks(int64_t rows, int xs) {
  return (unsigned)((((rows + PREP_R - 1) / PREP_R) * xs + 255) / 256);
}

// ---------------------------------------------------------------------------------------------------
// PPO head: mu = H3a W4a^T + b4a, v = H3c W4c^T + b4c, Normal(mu, std) log-prob / entropy, clipped
// surrogate, clipped value loss, KL(old || new) (ppo.py:98-147, actor_critic.py:126-135); gradient of
// loss = surrogate + c_v value - c_e entropy w.r.t. mu, v and std; dH3 = (dmu W4a | dv W4c) * elu'(H3);
// per-workgroup partials: dW4a, db4a, dW4c, db4c, dstd, sum kl, sum surrogate, sum value loss.
struct HeadArgs {
  const float* h3;      // [B][2*HW]: actor | critic
  float* dh3;           // [B][2*HW]
  const float *w4a, *b4a, *w4c, *b4c, *stdv;
  const float *actions, *old_mu, *old_sigma, *tv, *ret, *adv, *old_logp;
  const int64_t* rows;
  int B, na;
  float clip, ent_coef, vcoef;
  int clipped_value;
  float* part;          // [gridDim.x][part_len]
  int part_len;
};

// partial layout
__host__ __device__ constexpr int hp_w4a(int) { return 0; }
__host__ __device__ constexpr int hp_b4a(int na) { return na * HEAD_W; }
__host__ __device__ constexpr int hp_w4c(int na) { return na * HEAD_W + na; }
__host__ __device__ constexpr int hp_b4c(int na) { return na * HEAD_W + na + HEAD_W; }
__host__ __device__ constexpr int hp_std(int na) { return na * HEAD_W + na + HEAD_W + 1; }
__host__ __device__ constexpr int hp_kl(int na) { return na * HEAD_W + na + HEAD_W + 1 + na; }
__host__ __device__ constexpr int hp_len(int na) { return hp_kl(na) + 3; }  // kl, surrogate, value

// NA: the action count (12: the quadrupeds' joints; 3: the navigation policy's commands), rows of per-action values
// padded to NAP floats for the float4 reads; TANH: the bodies' activation (dH3 takes 1 - h^2 where ELU takes elu'(h))
template <int NA, bool TANH>
__global__ __launch_bounds__(HEAD_THREADS) void ppo_head_kernel(HeadArgs a) {
  // phases: (0) stage H3 / head weights and the minibatch rows' indices, then issue the gathered per-(row, action)
  // and per-row loads (old actions / mu / sigma, advantage, old log-prob, target value, return) so their latency
  // hides under (1) mu, v; (2) per (row, action): log-prob and KL terms  (3) per row: ratio, clipped surrogate,
  // clipped value loss, their gradients  (4) per (row, action): d loss / d mu, d loss / d std  (5) per column: dH3
  // and the head weight-gradient partials.  Two global round trips in all (rows, then the gathered rows).
  // pitch 4 (mod 32) floats: the row-per-lane float4 reads of (1) hit distinct banks in every 8-lane group
  constexpr int HP = 2 * HEAD_W + 4;
  constexpr int NAP = (NA + 3) / 4 * 4;
  static_assert(NA <= 16 && HEAD_W % 16 == 0, "float4 rows");  // (t < NA, t == 16 and t >= 32 share the last phase)
  constexpr int NG = (HEAD_ROWS * NA + HEAD_THREADS - 1) / HEAD_THREADS;  // gathered (row, action) items per thread
  __shared__ __attribute__((aligned(16))) float H[HEAD_ROWS][HP];
  __shared__ __attribute__((aligned(16))) float W4[NA + 1][HEAD_W];
  __shared__ float MU[HEAD_ROWS][NA + 1];   // mu_j, then d = a_j - mu_j
  __shared__ float VP[HEAD_ROWS][8];
  __shared__ __attribute__((aligned(16))) float LP[HEAD_ROWS][NAP];  // log-prob term, then d loss / d mu
  __shared__ float KT[HEAD_ROWS][NA];       // KL term, then d loss / d std
  __shared__ float DR[HEAD_ROWS][2];        // d loss / d logp, d loss / d v
  __shared__ float SC[HEAD_ROWS][3];        // kl, surrogate, value loss per row
  __shared__ float SD[3][NA];               // std, log std, 1/std^2
  __shared__ float GA[3][HEAD_ROWS][NA];    // gathered old actions, old mu, old sigma
  __shared__ float GR[4][HEAD_ROWS];        // gathered advantage, old log-prob, target value, return
  __shared__ int64_t RW[HEAD_ROWS];
  const int t = threadIdx.x;
  const int r0 = blockIdx.x * HEAD_ROWS;
  const int nrows = min(HEAD_ROWS, a.B - r0);
  if (t < HEAD_ROWS) RW[t] = t < nrows ? a.rows[r0 + t] : a.rows[r0];
  if (t < NA) {
    const float sd = a.stdv[t];
    SD[0][t] = sd;
    SD[1][t] = logf(sd);
    SD[2][t] = 1.f / (sd * sd);
  }
  {
    constexpr int NV = HEAD_ROWS * 2 * HEAD_W / 4 / HEAD_THREADS;
    float4 v[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int i = t + u * HEAD_THREADS, r = i / (HEAD_W / 2), c = 4 * (i % (HEAD_W / 2));
      v[u] = r < nrows ? *reinterpret_cast<const float4*>(a.h3 + (int64_t)(r0 + r) * (2 * HEAD_W) + c)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int i = t + u * HEAD_THREADS, r = i / (HEAD_W / 2), c = 4 * (i % (HEAD_W / 2));
      *reinterpret_cast<float4*>(&H[r][c]) = v[u];
    }
  }
  for (int i = t; i < (NA + 1) * HEAD_W; i += HEAD_THREADS) {
    const int j = i / HEAD_W, k = i - j * HEAD_W;
    W4[j][k] = j < NA ? a.w4a[j * HEAD_W + k] : a.w4c[k];
  }
  __syncthreads();
  // (0b) the gathered loads, all issued before (1) uses none of them
  float ga[3][NG], gr = 0.f;
#pragma unroll
  for (int u = 0; u < NG; ++u) {
    const int i = t + u * HEAD_THREADS;
    const int r = i / NA, j = i - r * NA;
    const bool ok = i < HEAD_ROWS * NA;
    const int64_t o = RW[ok ? r : 0] * NA + j;
    ga[0][u] = ok ? a.actions[o] : 0.f;
    ga[1][u] = ok ? a.old_mu[o] : 0.f;
    ga[2][u] = ok ? a.old_sigma[o] : 1.f;
  }
  if (t < 4 * HEAD_ROWS) {
    const int q = t / HEAD_ROWS, r = t - q * HEAD_ROWS;
    const float* src = q == 0 ? a.adv : q == 1 ? a.old_logp : q == 2 ? a.tv : a.ret;
    gr = src[RW[r]];
  }
  // (1) thread (r, q): actions q, q+8 and an eighth of the value dot (float4 LDS reads, the same sequential fmaf
  // order over k as one element at a time)
  {
    const int r = t & (HEAD_ROWS - 1), q = t / HEAD_ROWS;
    const float4* hr = reinterpret_cast<const float4*>(&H[r][0]);
    auto dot4 = [](float s, float4 h, float4 w) {
      s = fmaf(h.x, w.x, s);
      s = fmaf(h.y, w.y, s);
      s = fmaf(h.z, w.z, s);
      return fmaf(h.w, w.w, s);
    };
    for (int j = q; j < NA; j += 8) {
      const float4* wr = reinterpret_cast<const float4*>(&W4[j][0]);
      float s = 0.f;
#pragma unroll 8
      for (int k4 = 0; k4 < HEAD_W / 4; ++k4) s = dot4(s, hr[k4], wr[k4]);
      MU[r][j] = s + a.b4a[j];
    }
    const float4* wv = reinterpret_cast<const float4*>(&W4[NA][q * (HEAD_W / 8)]);
    const float4* hv = hr + (HEAD_W + q * (HEAD_W / 8)) / 4;
    float s = 0.f;
#pragma unroll
    for (int k4 = 0; k4 < HEAD_W / 32; ++k4) s = dot4(s, hv[k4], wv[k4]);
    VP[r][q] = s;
  }
#pragma unroll
  for (int u = 0; u < NG; ++u) {
    const int i = t + u * HEAD_THREADS;
    if (i < HEAD_ROWS * NA) {
      const int r = i / NA, j = i - r * NA;
      GA[0][r][j] = ga[0][u];
      GA[1][r][j] = ga[1][u];
      GA[2][r][j] = ga[2][u];
    }
  }
  if (t < 4 * HEAD_ROWS) GR[t / HEAD_ROWS][t & (HEAD_ROWS - 1)] = gr;
  __syncthreads();
  // (2) per (row, action): Normal log-prob term and KL(old || new) term (ppo.py:111-114)
  for (int i = t; i < HEAD_ROWS * NA; i += HEAD_THREADS) {
    const int r = i / NA, j = i - r * NA;
    float lp = 0.f, kt = 0.f, d = 0.f;
    if (r < nrows) {
      const float s = SD[0][j], mu = MU[r][j];
      d = GA[0][r][j] - mu;
      lp = -(d * d) / (2.f * (s * s)) - SD[1][j] - LOG_SQRT_2PI;
      const float so = GA[2][r][j], dm = GA[1][r][j] - mu;
      kt = logf(s / so + 1.e-5f) + (so * so + dm * dm) / (2.f * (s * s)) - 0.5f;
    }
    MU[r][j] = d;
    LP[r][j] = lp;
    KT[r][j] = kt;
  }
  __syncthreads();
  const float invB = 1.f / (float)a.B;
  // (3) per row
  if (t < HEAD_ROWS) {
    const int r = t;
    float kl = 0.f, surr_loss = 0.f, vloss = 0.f, dv = 0.f, dlogp = 0.f;
    if (r < nrows) {
      const float v = (((VP[r][0] + VP[r][1]) + (VP[r][2] + VP[r][3])) + ((VP[r][4] + VP[r][5]) + (VP[r][6] + VP[r][7]))) +
                      a.b4c[0];
      float logp = 0.f;
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        logp += LP[r][j];
        kl += KT[r][j];
      }
      const float adv = GR[0][r];
      const float ratio = expf(logp - GR[1][r]);
      const float surr = -adv * ratio;
      const float rc = fminf(fmaxf(ratio, 1.f - a.clip), 1.f + a.clip);
      const float surr_c = -adv * rc;
      surr_loss = fmaxf(surr, surr_c);
      // torch.max backward: the larger side takes the gradient, ties split it in half
      const float ga = surr > surr_c ? invB : (surr == surr_c ? 0.5f * invB : 0.f);
      const float gb = surr_c > surr ? invB : (surr == surr_c ? 0.5f * invB : 0.f);
      const bool in_rng = ratio >= 1.f - a.clip && ratio <= 1.f + a.clip;
      const float dratio = -adv * ga + (in_rng ? -adv * gb : 0.f);
      dlogp = dratio * ratio;
      // value loss (ppo.py:133-143)
      const float tv = GR[2][r], ret = GR[3][r];
      const float gv = a.vcoef * invB;
      if (a.clipped_value) {
        const float dvt = v - tv;
        const float vc = tv + fminf(fmaxf(dvt, -a.clip), a.clip);
        const float l1 = (v - ret) * (v - ret), l2 = (vc - ret) * (vc - ret);
        vloss = fmaxf(l1, l2);
        const float g1 = l1 > l2 ? gv : (l1 == l2 ? 0.5f * gv : 0.f);
        const float g2 = l2 > l1 ? gv : (l1 == l2 ? 0.5f * gv : 0.f);
        const bool vin = dvt >= -a.clip && dvt <= a.clip;
        dv = g1 * 2.f * (v - ret) + (vin ? g2 * 2.f * (vc - ret) : 0.f);
      } else {
        vloss = (ret - v) * (ret - v);
        dv = gv * 2.f * (v - ret);
      }
    }
    DR[r][0] = dlogp;
    DR[r][1] = dv;
    SC[r][0] = kl;
    SC[r][1] = surr_loss;
    SC[r][2] = vloss;
  }
  __syncthreads();
  // (4) per (row, action): d/d mu = dlogp (a - mu)/var; d/d std = dlogp ((a-mu)^2/var - 1)/std - c_e/(B std)
  for (int i = t; i < HEAD_ROWS * NA; i += HEAD_THREADS) {
    const int r = i / NA, j = i - r * NA;
    float dm = 0.f, ds = 0.f;
    if (r < nrows) {
      const float d = MU[r][j], dl = DR[r][0], s = SD[0][j], ivar = SD[2][j];
      dm = dl * (d * ivar);
      ds = dl * (d * d * ivar - 1.f) / s - a.ent_coef * invB / s;
    }
    LP[r][j] = dm;
    KT[r][j] = ds;
  }
  __syncthreads();
  // (5) backward into H3 and the head weight-gradient partials: thread = column of [actor | critic]
  float* P = a.part + (int64_t)blockIdx.x * a.part_len;
  {
    const int k = t;  // 0..255
    if (k < HEAD_W) {
      float wk[NA], accw[NA];
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        wk[j] = W4[j][k];
        accw[j] = 0.f;
      }
#pragma unroll 2
      for (int r = 0; r < nrows; ++r) {
        const float h = H[r][k];
        float dmr[NAP];  // (row r's d loss / d mu: NAP / 4 broadcast float4 reads; columns past NA are not used)
#pragma unroll
        for (int j4 = 0; j4 < NAP / 4; ++j4) {
          const float4 v = reinterpret_cast<const float4*>(&LP[r][0])[j4];
          dmr[4 * j4] = v.x; dmr[4 * j4 + 1] = v.y; dmr[4 * j4 + 2] = v.z; dmr[4 * j4 + 3] = v.w;
        }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
          const float dm = dmr[j];
          s = fmaf(dm, wk[j], s);
          accw[j] = fmaf(dm, h, accw[j]);
        }
        a.dh3[(int64_t)(r0 + r) * (2 * HEAD_W) + k] = s * (TANH ? 1.f - h * h : delu(h));
      }
#pragma unroll
      for (int j = 0; j < NA; ++j) P[hp_w4a(NA) + j * HEAD_W + k] = accw[j];
    } else {
      const int kk = k - HEAD_W;
      const float wk = W4[NA][kk];
      float accc = 0.f;
      for (int r = 0; r < nrows; ++r) {
        const float h = H[r][k];
        const float d = DR[r][1];
        accc = fmaf(d, h, accc);
        a.dh3[(int64_t)(r0 + r) * (2 * HEAD_W) + k] = (d * wk) * (TANH ? 1.f - h * h : delu(h));
      }
      P[hp_w4c(NA) + kk] = accc;
    }
  }
  if (t < NA) {
    float sb = 0.f, ss = 0.f;
    for (int r = 0; r < nrows; ++r) {
      sb += LP[r][t];
      ss += KT[r][t];
    }
    P[hp_b4a(NA) + t] = sb;
    P[hp_std(NA) + t] = ss;
  } else if (t == 16) {
    float sb = 0.f;
    for (int r = 0; r < nrows; ++r) sb += DR[r][1];
    P[hp_b4c(NA)] = sb;
  } else if (t >= 32 && t < 35) {
    const int c = t - 32;
    float s = 0.f;
    for (int r = 0; r < nrows; ++r) s += SC[r][c];
    P[hp_kl(NA) + c] = s;
  }
}

// ---------------------------------------------------------------------------------------------------
// Rollout head of PPO.act (ppo.py:62-74, actor_critic.py:126-135,170-173): mu = H3a W4a^T + b,
// value = H3c W4c^T + b, a = mu + std * eps (eps injected or Box-Muller on the counter RNG), log-prob,
// and the transition row of RolloutStorage.add_transitions (rollout_storage.py:57-71).
struct ActHeadArgs {
  const float* h3;  // [n][2*HW]
  const float *w4a, *b4a, *w4c, *b4c, *stdv;
  const float *obs, *priv, *hist, *eps;
  int n, na, no, np;
  uint64_t seed, counter;
  int64_t row_offset;  // global id of row 0 (the rank's env_offset): the noise key, so draws do not depend on sharding
  float *actions, *mu, *values, *logp;
  lrl_rollout_store store;
  int store_row, do_store;
  float* xa_out;  // ENC_ONLY: the [obs | latent | 0] rows, pitch xs
  float* hist_shift;  // == hist, writable: the storage copy also shifts the rows left by hist_slot floats (else NULL)
  int hist_slot;
};

// rows [0, nrows) of src (pitch sld) -> dst (pitch dld), `cols` floats each, by the block's NT
// threads with 8 loads in flight per thread (float2 when both sides allow)
template <int NT = HEAD_THREADS>
__device__ __forceinline__ void copy_rows(const float* __restrict__ src, int64_t sld, float* __restrict__ dst,
                                          int64_t dld, int nrows, int cols, int t) {
  if (((((uintptr_t)src | (uintptr_t)dst) & 7) == 0) && (((sld | dld | cols) & 1) == 0)) {
    const int c2 = cols / 2, n = nrows * c2;
    for (int i0 = t; i0 < n; i0 += 8 * NT) {
      float2 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * NT, r = i / c2, c = i - r * c2;
        if (i < n) v[u] = reinterpret_cast<const float2*>(src + r * sld)[c];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * NT, r = i / c2, c = i - r * c2;
        if (i < n) reinterpret_cast<float2*>(dst + r * dld)[c] = v[u];
      }
    }
  } else {
    const int n = nrows * cols;
    for (int i0 = t; i0 < n; i0 += 8 * NT) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * NT, r = i / cols, c = i - r * cols;
        if (i < n) v[u] = src[r * sld + c];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * NT, r = i / cols, c = i - r * cols;
        if (i < n) dst[r * dld + c] = v[u];
      }
    }
  }
}

// copy_rows that also shifts the source rows left by one slot in place: every loaded value goes to dst as in
// copy_rows and, from column `slot` on, to src[r][c - slot] (the HistoryWrapper shift, hist[:, :cols - slot] =
// hist[:, slot:]; the newest slot src[r][cols - slot:] is not written).  src and dst pitches as copy_rows'.
// The shifted store of element i lands on element i - slot of the same row, which another thread — of another wave,
// or of an earlier batch — loads.  So a batch's stores are issued only once every wave's loads of that batch have
// returned: each wave waits on its own loads (vmcnt(0): a barrier alone lets a wave pass with loads in flight) and
// then meets the workgroup at the barrier.  A store reaches only elements at or below its batch, never the next
// batch's, so one barrier per batch is enough.  Every thread of the workgroup calls this with the same arguments
// (the batch loop is uniform: its barrier is reached by all NT threads).
template <int NT = HEAD_THREADS>
__device__ __forceinline__ void copy_rows_shift(float* src, int64_t sld, float* dst, int64_t dld, int nrows, int cols,
                                                int slot, int t) {
  if (((((uintptr_t)src | (uintptr_t)dst) & 7) == 0) && (((sld | dld | cols | slot) & 1) == 0)) {
    const int c2 = cols / 2, s2 = slot / 2, n = nrows * c2;
    for (int b0 = 0; b0 < n; b0 += 8 * NT) {
      float2 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = b0 + t + u * NT, r = i / c2, c = i - r * c2;
        if (i < n) v[u] = reinterpret_cast<const float2*>(src + r * sld)[c];
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = b0 + t + u * NT, r = i / c2, c = i - r * c2;
        if (i < n) {
          reinterpret_cast<float2*>(dst + r * dld)[c] = v[u];
          if (c >= s2) reinterpret_cast<float2*>(src + r * sld)[c - s2] = v[u];
        }
      }
    }
  } else {
    const int n = nrows * cols;
    for (int b0 = 0; b0 < n; b0 += 8 * NT) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = b0 + t + u * NT, r = i / cols, c = i - r * cols;
        if (i < n) v[u] = src[r * sld + c];
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = b0 + t + u * NT, r = i / cols, c = i - r * cols;
        if (i < n) {
          dst[r * dld + c] = v[u];
          if (c >= slot) src[r * sld + c - slot] = v[u];
        }
      }
    }
  }
}

// One (row g, action j) of the rollout head: the noise (injected, or Box-Muller on the counter RNG, stream POLICY, keyed
// by the global env id: pairs of actions share one Philox draw), the action into `act`; returns the log-prob term
__device__ __forceinline__ float act_draw(const float* eps, int64_t row_offset, uint64_t seed, uint64_t counter, int g,
                                          int j, int na, float m, float sd, float& act) {
  float e;
  if (eps) {
    e = eps[(int64_t)g * na + j];
  } else {
    lrl_u32x4 u = lrl_philox((uint32_t)(row_offset + g), (uint32_t)counter, (LRL_RNG_POLICY << 16) ^ (uint32_t)(counter >> 32),
                             (uint32_t)(j >> 1), seed);
    const float u1 = fmaxf(lrl_u01(u.v[0]), 1e-7f), u2 = lrl_u01(u.v[1]);
    const float rad = sqrtf(-2.f * logf(u1)), th = 6.283185307179586f * u2;
    e = (j & 1) ? rad * sinf(th) : rad * cosf(th);
  }
  act = m + sd * e;
  const float d = act - m;
  return -(d * d) / (2.f * (sd * sd)) - logf(sd) - LOG_SQRT_2PI;
}

// rollout head: ACT_ROWS rows per workgroup (4096 envs -> 256 workgroups, one per CU: the kernel holds one workgroup
// per CU (its register footprint), so 512 eight-row workgroups ran in two rounds — 18.3 against 13.7 us; 32 rows 20.7 us)
constexpr int ACT_ROWS = 16, ACT_Q = HEAD_THREADS / ACT_ROWS;  // 16 thread groups per row
__global__ __launch_bounds__(HEAD_THREADS) void act_head_kernel(ActHeadArgs a) {
  constexpr int HP = 2 * HEAD_W + 1;
  __shared__ float H[ACT_ROWS][HP];
  __shared__ float W4[MAX_ACT + 1][HEAD_W];
  __shared__ float MU[ACT_ROWS][MAX_ACT + 1];
  __shared__ float VP[ACT_ROWS][ACT_Q];
  const int t = threadIdx.x, na = a.na;
  const int r0 = blockIdx.x * ACT_ROWS;
  const int nrows = min(ACT_ROWS, a.n - r0);
  {
    constexpr int NV = ACT_ROWS * 2 * HEAD_W / 4 / HEAD_THREADS;
    float4 v[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int i = t + u * HEAD_THREADS, r = i / (HEAD_W / 2), c = 4 * (i % (HEAD_W / 2));
      v[u] = r < nrows ? *reinterpret_cast<const float4*>(a.h3 + (int64_t)(r0 + r) * (2 * HEAD_W) + c)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int i = t + u * HEAD_THREADS, r = i / (HEAD_W / 2), c = 4 * (i % (HEAD_W / 2));
      *reinterpret_cast<float4*>(&H[r][c]) = v[u];
    }
  }
  for (int i = t; i < (na + 1) * HEAD_W; i += HEAD_THREADS) {
    const int j = i / HEAD_W, k = i - j * HEAD_W;
    W4[j][k] = j < na ? a.w4a[j * HEAD_W + k] : a.w4c[k];
  }
  __syncthreads();
  {
    const int r = t & (ACT_ROWS - 1), q = t / ACT_ROWS;
    for (int j = q; j < na; j += ACT_Q) {
      float s = 0.f;
      for (int k = 0; k < HEAD_W; ++k) s = fmaf(H[r][k], W4[j][k], s);
      MU[r][j] = s + a.b4a[j];
    }
    float s = 0.f;
    for (int k = q * (HEAD_W / ACT_Q); k < (q + 1) * (HEAD_W / ACT_Q); ++k) s = fmaf(H[r][HEAD_W + k], W4[na][k], s);
    VP[r][q] = s;
  }
  __syncthreads();
  const int64_t so = (int64_t)a.store_row * a.n;
  // one thread per (row, action): sample + write; the per-row log-prob sum is formed after a barrier
  for (int i = t; i < nrows * na; i += HEAD_THREADS) {
    const int r = i / na, j = i - r * na, g = r0 + r;
    const float m = MU[r][j], sd = a.stdv[j];
    float act;
    MU[r][j] = act_draw(a.eps, a.row_offset, a.seed, a.counter, g, j, na, m, sd, act);  // (mu no longer needed)
    a.actions[(int64_t)g * na + j] = act;
    if (a.mu) a.mu[(int64_t)g * na + j] = m;
    if (a.do_store) {
      const int64_t o = (so + g) * na + j;
      a.store.actions[o] = act;
      a.store.mu[o] = m;
      a.store.sigma[o] = sd;
    }
  }
  __syncthreads();
  if (t < nrows) {
    const int g = r0 + t;
    float lp = 0.f;
    for (int j = 0; j < na; ++j) lp += MU[t][j];
    float vs[ACT_Q];
#pragma unroll
    for (int q = 0; q < ACT_Q; ++q) vs[q] = VP[t][q];
#pragma unroll
    for (int w = ACT_Q / 2; w >= 1; w /= 2)  // pairwise tree, fixed order
#pragma unroll
      for (int q = 0; q < w; ++q) vs[q] = vs[2 * q] + vs[2 * q + 1];
    const float v = vs[0] + a.b4c[0];
    if (a.values) a.values[g] = v;
    if (a.logp) a.logp[g] = lp;
    if (a.do_store) {
      a.store.values[so + g] = v;
      a.store.logp[so + g] = lp;
    }
  }
  if (a.do_store) {  // obs / priv / history rows of this tile into storage row `store_row`
    const int64_t b = so + r0;
    copy_rows(a.obs + (int64_t)r0 * a.no, a.no, a.store.obs + b * a.no, a.no, nrows, a.no, t);
    if (a.priv)  // (NULL: a plain net acting without privileged observations)
      copy_rows(a.priv + (int64_t)r0 * a.np, a.np, a.store.priv + b * a.np, a.np, nrows, a.np, t);
    if (a.hist && a.store.hist) {
      const int hd = a.store.hist_dim, ld = a.store.hist_ld > hd ? a.store.hist_ld : hd;
      if (a.hist_shift) copy_rows_shift(a.hist_shift + (int64_t)r0 * hd, hd, a.store.hist + b * ld, ld, nrows, hd, a.hist_slot, t);
      else copy_rows(a.hist + (int64_t)r0 * hd, hd, a.store.hist + b * ld, ld, nrows, hd, t);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// Fused rollout act (PPO.act, ppo.py:62-74 -> actor_critic.py:137-147,170-173, + RolloutStorage.add_transitions,
// rollout_storage.py:57-71), act_fused_kernel, in two instances:
//  * ENC_ONLY: the GEMM chain's first launch.  One workgroup carries FA_R = 16 env rows through the obs staging and
//    the env-factor encoder and writes the X rows [obs | latent | 0] for the x6 products behind it.
//  * the whole act in one launch.  One workgroup carries (a tile of OA_R = 32 env rows, one group: actor or critic)
//    through the encoder, its group's body, its head and its share of the storage row, with every activation in LDS:
//    no activation goes to global memory and a rollout step's act is one launch instead of five.
// The encoder runs on the fp32 MFMA (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation, k-sequential): a
// wave owns a run of 16-column output tiles; per 32-k chunk lane (i, q) = (lane & 15, lane >> 4) reads
// A[i][k0 + 8q .. +7] from LDS and, per tile, the 8 weights W[n][k0 + 8q .. +7] of its output column n straight from L2
// (FA_D chunks in flight); the 32-row instance multiplies both 16-row blocks against each weight register set.
// The bodies of the one-launch act run as the chain's x6 products do (lrl_gemm.hip): every operand element split into
// hi / mid / lo bf16 parts, 16-k steps from k = 0, x6_mma's six products per step, epi_apply<EPI_BIAS_ELU> — so each
// output goes through the chain's instruction sequence and has its bits.  The activations (X, H1, H2) live in LDS as
// plane images in gemm_x6_kernel's layout ([32][16] bf16 per plane and 16-k slice, x6_off), so an A operand is one
// ds_read_b128 per plane and a layer needs no barrier inside it; a wave owns a run of 32-column output tiles and reads
// its B operand — fp32 weights W[n][k], each element used by this wave only — from L2 into registers, splits it there
// and feeds x6_mma (oa_tiles).  H3 is written as fp32 for the heads.
constexpr int FA_R = 16, FA_THREADS = 256;  // ENC_ONLY: rows and threads per workgroup
constexpr int FA_D = 2;       // weight chunks (32 k each) in flight per wave: the L2 round trip over the MFMA work
constexpr int FA_XP = 260;    // X / he1 pitch (widths <= 256) + 4: conflict-free b128 row reads
constexpr int FA_ENC_MIDP = 260;  // priv [R][36] / he2 [R][enc_h1 + 4 <= 260]
constexpr int FA_ENC_LDS_FLOATS = FA_R * (FA_XP + FA_XP + FA_ENC_MIDP);  // ENC_ONLY: X, he1, priv / he2 (49.9 KB)
// The one-launch act's LDS (bytes; one extern array):
//   region A [0, OA_A_BYTES): H1 planes (32 x ac_h0 <= 512, 6 B per element); before them the encoder's X / he1 /
//     priv-he2 fp32 tiles (the last one ends 1.5 KB inside region B, dead before the X planes are written); after
//     them H3 [32][OA_H3P] fp32
//   region B [OA_A_BYTES, OA_LDS_BYTES): X planes (32 x xs <= 256), then H2 planes (32 x ac_h1 <= 256), then the
//     head's weight rows and its mu / value-partial tile
constexpr int OA_R = 32, OA_THREADS = 512;  // two waves per SIMD: one's MFMAs run under the other's split and ELU work
constexpr int OA_MAX_H0 = 512, OA_MAX_H1 = 256, OA_MAX_XS = 256;
constexpr int OA_PLANE = OA_R * XBK;    // bf16 elements of one plane image of a 16-k slice
constexpr int OA_SLICE = 3 * OA_PLANE;  // hi, mid, lo
constexpr int OA_A_BYTES = OA_R * OA_MAX_H0 * 6, OA_B_BYTES = OA_R * OA_MAX_H1 * 6;
constexpr int OA_LDS_BYTES = OA_A_BYTES + OA_B_BYTES;  // 144 KB: one workgroup per CU
constexpr int OA_H3P = HEAD_W + 1;  // H3 pitch: the heads read a row per lane
static_assert(OA_R * OA_MAX_XS * 6 <= OA_B_BYTES && OA_R * OA_H3P * 4 <= OA_A_BYTES, "overlays");
static_assert(OA_R * (2 * FA_XP + FA_ENC_MIDP) * 4 <= OA_A_BYTES + 2048, "encoder tiles");
static_assert(((HEAD_NA * HEAD_W) + 2 * OA_R * 16) * 4 <= OA_B_BYTES, "head scratch");

// Phase timers of the fused act (build with -DLRL_ACT_PROFILE, read with lrl_debug_act_profile): shader-clock cycles
// per phase summed over workgroups (thread 0's view): stage, enc1..3, X planes, ac1..3, heads, sampling, storage copies
#ifdef LRL_ACT_PROFILE
__device__ unsigned long long g_act_prof[12];
#define FA_PROF_INIT clock64()
#define FA_PROF(i)                                                  \
  if (threadIdx.x == 0) {                                           \
    const unsigned long long t_ = clock64();                        \
    atomicAdd(&g_act_prof[i], t_ - fa_t);                           \
    fa_t = t_;                                                      \
  }
#else
#define FA_PROF_INIT 0ull
#define FA_PROF(i)
#endif

typedef float fa_f32x4 __attribute__((ext_vector_type(4)));

struct FaLayer {
  const float* A;   // LDS input rows
  int pa, K;        // pitch, k extent (multiple of 32, zero-padded)
  const float* W;   // weights [Nw rows][ldw]
  int ldw, Kw, Nw;  // row pitch, valid k (< Kw), valid rows (< Nw)
  const float* b;   // bias
  float* C;         // LDS output: column n at C[row * pc + coff + n]
  int pc, coff, Ng; // Ng: Nw rounded up to whole 16-column tiles
  int elu;          // ELU after the bias
};

// NB column tiles from t0 for RB blocks of 16 rows; VEC: 16-B aligned weight rows (float4 loads), else dword loads.  The
// loads are branch-free (addresses clamped into the weights, out-of-range elements zeroed by selection) so the compiler
// keeps the FA_D chunks in flight with counted vmcnt waits instead of draining at every guarded load
template <int NB, bool VEC, int RB>
__device__ __forceinline__ void fa_tiles(const FaLayer& L, int t0) {
  const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
  const float* A = L.A + i * L.pa + 8 * q;
  const float* rowp[NB];
  bool rok[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int n = (t0 + j) * 16 + i;
    rok[j] = n < L.Nw;
    rowp[j] = L.W + (int64_t)(rok[j] ? n : L.Nw - 1) * L.ldw;
  }
  fa_f32x4 acc[RB][NB];
#pragma unroll
  for (int b = 0; b < RB; ++b)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[b][j] = fa_f32x4{0.f, 0.f, 0.f, 0.f};
  // per 32-k chunk lane (i, q) holds the 8 weights W[n][k0 + 8q .. +7] of each tile (a whole 128-B line per row and
  // chunk over the 4 lane groups) and A[i][k0 + 8q .. +7]; step s multiplies k = k0 + 8q + s
  auto load_b = [&](float4 (&bv)[NB][2], int k0) {
    const int k = k0 + 8 * q;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if constexpr (VEC) {  // (Kw % 4 == 0: a float4 is wholly inside or wholly outside the row)
        const int k1 = min(k, L.Kw - 4), k2 = min(k + 4, L.Kw - 4);
        float4 v0 = *reinterpret_cast<const float4*>(rowp[j] + k1);
        float4 v1 = *reinterpret_cast<const float4*>(rowp[j] + k2);
        const bool o0 = rok[j] && k < L.Kw, o1 = rok[j] && k + 4 < L.Kw;
        bv[j][0] = o0 ? v0 : make_float4(0.f, 0.f, 0.f, 0.f);
        bv[j][1] = o1 ? v1 : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float x = rowp[j][min(k + u, L.Kw - 1)];
          v[u] = (rok[j] && k + u < L.Kw) ? x : 0.f;
        }
        bv[j][0] = make_float4(v[0], v[1], v[2], v[3]);
        bv[j][1] = make_float4(v[4], v[5], v[6], v[7]);
      }
    }
  };
  // FA_D chunks of weights in flight (a ring of register sets, indexed at compile time by unrolling FA_D chunks)
  const int nck = L.K >> 5;
  float4 ring[FA_D][NB][2];
#pragma unroll
  for (int d = 0; d < FA_D; ++d) load_b(ring[d], 32 * min(d, nck - 1));
  for (int c0 = 0; c0 < nck; c0 += FA_D) {
#pragma unroll
    for (int d = 0; d < FA_D; ++d) {
      const int c = c0 + d;
      if (c < nck) {
        float av[RB][8];
#pragma unroll
        for (int b = 0; b < RB; ++b) {
          const float4 a0 = *reinterpret_cast<const float4*>(A + 16 * b * L.pa + 32 * c);
          const float4 a1 = *reinterpret_cast<const float4*>(A + 16 * b * L.pa + 32 * c + 4);
          av[b][0] = a0.x; av[b][1] = a0.y; av[b][2] = a0.z; av[b][3] = a0.w;
          av[b][4] = a1.x; av[b][5] = a1.y; av[b][6] = a1.z; av[b][7] = a1.w;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const float4& bq = ring[d][j][u >> 2];
            const float bw = (u & 3) == 0 ? bq.x : (u & 3) == 1 ? bq.y : (u & 3) == 2 ? bq.z : bq.w;
#pragma unroll
            for (int b = 0; b < RB; ++b) acc[b][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[b][u], bw, acc[b][j], 0, 0, 0);
          }
        }
        load_b(ring[d], 32 * min(c + FA_D, nck - 1));  // (past the end: a harmless re-read of the last chunk)
      }
    }
  }
  // C/D: column i of the tile, rows 4q .. 4q + 3 of each 16-row block in the four registers
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int n = (t0 + j) * 16 + i;
    if (n < L.Nw) {
      const float bias = L.b[n];
#pragma unroll
      for (int b = 0; b < RB; ++b) {
        float* c = L.C + (16 * b + 4 * q) * L.pc + L.coff + n;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[b][j][r] + bias;
          if (L.elu) v = v > 0.f ? v : expm1f(v);
          c[r * L.pc] = v;
        }
      }
    }
  }
}

// one layer: the T = Ng / 16 column tiles split into equal runs over the workgroup's NW = 4 * RB waves (T < NW: one
// tile per wave).  NBC > 0: the run length known at compile time (the presets' widths), else dispatched on it
template <int NBC, bool VEC, int RB>
__device__ __forceinline__ void fa_layer(const FaLayer& L) {
  constexpr int NW = 4 * RB;
  const int w = threadIdx.x >> 6, T = L.Ng >> 4;
  const int tpw = T >= NW ? T / NW : 1;
  if (w * tpw >= T) return;
  const int t0 = w * tpw;
  if constexpr (NBC > 0) {
    fa_tiles<NBC, VEC, RB>(L, t0);
  } else {
    switch (tpw) {
      case 1: fa_tiles<1, VEC, RB>(L, t0); break;
      case 2: fa_tiles<2, VEC, RB>(L, t0); break;
      case 4: fa_tiles<4, VEC, RB>(L, t0); break;
      default:
        for (int t = t0; t < t0 + tpw; ++t) fa_tiles<1, VEC, RB>(L, t);
    }
  }
}

struct FusedActArgs {
  const float* w;
  lrl_ppo_net net;
  const float *obs, *priv, *hist, *eps;
  int n, xs;
  uint32_t vec;  // bit l: float4 weight loads allowed for layer l (e2, e3, w1, w2, w3 = bits 1 .. 5)
  uint64_t seed, counter;
  int64_t row_offset;
  float *actions, *mu, *values, *logp;
  lrl_rollout_store store;
  int store_row, do_store;
  float* xa_out;  // ENC_ONLY: the [obs | latent | 0] rows, pitch xs
  float* hist_shift;  // == hist, writable: the storage copy also shifts the rows left by hist_slot floats (else NULL)
  int hist_slot;
};

// Obs staging and the env-factor encoder for 16 * RB rows from r0: X = [obs | latent | 0] (pitch FA_XP, zero rows past
// n), through he1 [.][FA_XP] and MID (priv [.][36], then he2 [.][enc_h1 + 4]).  Ends behind a barrier.
template <bool PRESET, int RB>
__device__ __forceinline__ void fa_encoder(const FusedActArgs& a, float* X, float* HE1, float* MID, int r0, int nrows,
                                           unsigned long long& fa_t) {
  constexpr int R = 16 * RB, NT = 256 * RB;  // (the 32-row instance runs in the one-launch act's 512 threads)
  const lrl_ppo_net& nt = a.net;
  const int t = threadIdx.x;
  const int no = nt.num_obs, np = nt.num_priv, PP = 36, EP2 = nt.enc_h1 + 4;
  // stage obs (zero padding and rows past n) and priv (k padded to 32)
  for (int e = t; e < R * a.xs; e += NT) {
    const int r = e / a.xs, c = e - r * a.xs;
    X[r * FA_XP + c] = (r < nrows && c < no) ? a.obs[(int64_t)(r0 + r) * no + c] : 0.f;
  }
  for (int e = t; e < R * 32; e += NT) {
    const int r = e >> 5, c = e & 31;
    MID[r * PP + c] = (r < nrows && c < np) ? a.priv[(int64_t)(r0 + r) * np + c] : 0.f;
  }
  __syncthreads();
  FA_PROF(0)
  const float* w = a.w;
  FaLayer L;
  // env_factor_encoder: priv -> enc_h0 (ELU) -> enc_h1 (ELU) -> latent, the latent into X[:, no:]
  L = FaLayer{MID, PP, 32, w + nt.e1w, np, np, nt.enc_h0, w + nt.e1b, HE1, FA_XP, 0, nt.enc_h0, 1};
  fa_layer<PRESET ? 4 / RB : 0, false, RB>(L);
  __syncthreads();
  FA_PROF(1)
  L = FaLayer{HE1, FA_XP, nt.enc_h0, w + nt.e2w, nt.enc_h0, nt.enc_h0, nt.enc_h1, w + nt.e2b, MID, EP2, 0, nt.enc_h1, 1};
  if (PRESET || (a.vec & 2u)) fa_layer<PRESET ? 2 / RB : 0, true, RB>(L);
  else fa_layer<0, false, RB>(L);
  __syncthreads();
  FA_PROF(2)
  L = FaLayer{MID, EP2, nt.enc_h1, w + nt.e3w, nt.enc_h1, nt.enc_h1, nt.latent, w + nt.e3b, X, FA_XP, no,
              (nt.latent + 15) / 16 * 16, 0};
  if (PRESET || (a.vec & 4u)) fa_layer<PRESET ? 1 : 0, true, RB>(L);
  else fa_layer<0, false, RB>(L);
  __syncthreads();
  FA_PROF(3)
}

// One body layer of the one-launch act for this workgroup's group and 32 rows
struct OaLayer {
  const uint16_t* A;  // LDS planes of the input: slice s (k = 16 s ..) at A + s * OA_SLICE, plane pl at + pl * OA_PLANE
  int K;              // k extent: a multiple of 32, the input zero from Kw on
  const float* W;     // the group's weights [N][ldw]
  int ldw, Kw, N;     // row pitch, valid k (< Kw), output width (a multiple of 32)
  const float* b;     // the group's bias
  uint16_t* Cp;       // LDS planes of the output, or nullptr:
  float* Cf;          // fp32 output rows, pitch OA_H3P
};

// NB 32-column output tiles from t0, D 32-k chunks of weights in flight.  Per chunk lane (li, h) = (lane & 31, lane >> 5)
// holds, per tile, W[n][k0 + 8h .. +7] (step 0) and W[n][k0 + 16 + 8h .. +7] (step 1) of its output column n:
// gemm_x6_kernel's operand element for that lane, so a row's 128-B line is consumed whole over the chunk's two steps.
// MODE 2: 16-B aligned weight rows of whole 32-k chunks (Kw = K; N is whole tiles): plain float4 loads; 1: 16-B aligned
// rows, 0: dword loads — both branch-free with clamped addresses and out-of-range elements zeroed by selection, as fa_tiles
template <int NB, int D, int MODE>
__device__ __forceinline__ void oa_tiles(const OaLayer& L, int t0) {
  const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
  const float* rowp[NB];
  bool rok[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int n = (t0 + j) * 32 + li;
    rok[j] = n < L.N;
    rowp[j] = L.W + (int64_t)(rok[j] ? n : L.N - 1) * L.ldw;
  }
  f32x16 acc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  auto load_b = [&](float4 (&bv)[NB][4], int k0) {
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int k = k0 + 16 * s + 8 * h;
        if constexpr (MODE == 2) {
          bv[j][2 * s] = *reinterpret_cast<const float4*>(rowp[j] + k);
          bv[j][2 * s + 1] = *reinterpret_cast<const float4*>(rowp[j] + k + 4);
        } else if constexpr (MODE == 1) {  // (Kw % 4 == 0: a float4 is wholly inside or wholly outside the row)
          const int k1 = min(k, L.Kw - 4), k2 = min(k + 4, L.Kw - 4);
          float4 v0 = *reinterpret_cast<const float4*>(rowp[j] + k1);
          float4 v1 = *reinterpret_cast<const float4*>(rowp[j] + k2);
          const bool o0 = rok[j] && k < L.Kw, o1 = rok[j] && k + 4 < L.Kw;
          bv[j][2 * s] = o0 ? v0 : make_float4(0.f, 0.f, 0.f, 0.f);
          bv[j][2 * s + 1] = o1 ? v1 : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          float v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const float x = rowp[j][min(k + u, L.Kw - 1)];
            v[u] = (rok[j] && k + u < L.Kw) ? x : 0.f;
          }
          bv[j][2 * s] = make_float4(v[0], v[1], v[2], v[3]);
          bv[j][2 * s + 1] = make_float4(v[4], v[5], v[6], v[7]);
        }
      }
  };
  const int nck = L.K >> 5;
  const uint16_t* Ap = L.A + x6_off(li, h);
  float4 ring[D][NB][4];
#pragma unroll
  for (int d = 0; d < D; ++d) load_b(ring[d], 32 * min(d, nck - 1));
  for (int c0 = 0; c0 < nck; c0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int c = c0 + d;
      if (c < nck) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8_t av[3];
#pragma unroll
          for (int pl = 0; pl < 3; ++pl)
            av[pl] = *reinterpret_cast<const bf16x8_t*>(Ap + (2 * c + s) * OA_SLICE + pl * OA_PLANE);
#pragma unroll
          for (int j = 0; j < NB; ++j) {
            const float4 x0 = ring[d][j][2 * s], x1 = ring[d][j][2 * s + 1];
            uint32_t hh[4], mm[4], ll[4];
            x6_split2(x0.x, x0.y, hh[0], mm[0], ll[0]);
            x6_split2(x0.z, x0.w, hh[1], mm[1], ll[1]);
            x6_split2(x1.x, x1.y, hh[2], mm[2], ll[2]);
            x6_split2(x1.z, x1.w, hh[3], mm[3], ll[3]);
            uint4 vh = make_uint4(hh[0], hh[1], hh[2], hh[3]), vm = make_uint4(mm[0], mm[1], mm[2], mm[3]),
                  vl = make_uint4(ll[0], ll[1], ll[2], ll[3]);
            bf16x8_t bv[3];
            bv[0] = *reinterpret_cast<bf16x8_t*>(&vh);
            bv[1] = *reinterpret_cast<bf16x8_t*>(&vm);
            bv[2] = *reinterpret_cast<bf16x8_t*>(&vl);
            acc[j] = x6_mma(av, bv, acc[j]);
          }
        }
        load_b(ring[d], 32 * min(c + D, nck - 1));  // (past the end: a harmless re-read of the last chunk)
      }
    }
  }
  // C/D: column li of the tile, rows 8q + 4h .. +3 in accumulator registers 4q .. 4q + 3 (gemm_x6_kernel's epilogue)
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int n = (t0 + j) * 32 + li;
    if (n < L.N) {
      const float bj = L.b[n];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row0 = 8 * q + 4 * h;
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = epi_apply<EPI_BIAS_ELU>(acc[j][4 * q + r], bj, 0.f);
        if (L.Cp) {  // element (row, k = n) of the next layer's A planes
          uint16_t* cp = L.Cp + (n >> 4) * OA_SLICE + (n & 7);
#pragma unroll
          for (int r = 0; r < 4; r += 2) {
            uint32_t hh, mm, ll;
            x6_split2(v[r], v[r + 1], hh, mm, ll);
            const int o0 = x6_off(row0 + r, (n >> 3) & 1), o1 = x6_off(row0 + r + 1, (n >> 3) & 1);
            cp[o0] = (uint16_t)hh;
            cp[o1] = (uint16_t)(hh >> 16);
            cp[OA_PLANE + o0] = (uint16_t)mm;
            cp[OA_PLANE + o1] = (uint16_t)(mm >> 16);
            cp[2 * OA_PLANE + o0] = (uint16_t)ll;
            cp[2 * OA_PLANE + o1] = (uint16_t)(ll >> 16);
          }
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) L.Cf[(row0 + r) * OA_H3P + n] = v[r];
        }
      }
    }
  }
}

// one body layer: the N / 32 column tiles split into runs over the 8 waves, a run taken two and one tile at a time
template <int MODE>
__device__ __forceinline__ void oa_layer(const OaLayer& L) {
  const int w = threadIdx.x >> 6, T = L.N >> 5, tpw = (T + 7) >> 3;
  int t = w * tpw;
  const int t1 = min(T, t + tpw);
  for (; t + 2 <= t1; t += 2) oa_tiles<2, 2, MODE>(L, t);
  if (t < t1) oa_tiles<1, 4, MODE>(L, t);
}

// PRESET: the presets' encoder (18 -> 256 -> 128 -> 18, aligned weights): every encoder layer's run length and load
// width fixed at compile time; otherwise dispatched per layer.
// ENC_ONLY: the rollout act's first four launches in one (ppo_prep_kernel's obs rows and the env-factor encoder's
// three products): the X rows [obs | latent | 0] go to a.xa_out for the actor / critic chain, in FA_ENC_LDS_FLOATS.
// Otherwise the whole act: workgroup b takes row tile b / 2 and group b % 2 (0 actor, 1 critic; neighbours in the grid
// sit on different XCDs, so an XCD's L2 serves one group's weights), in OA_LDS_BYTES
template <bool PRESET, bool ENC_ONLY = false>
__global__ __launch_bounds__(ENC_ONLY ? FA_THREADS : OA_THREADS) void act_fused_kernel(FusedActArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fa_lds[];
  unsigned long long fa_t = FA_PROF_INIT;
  const lrl_ppo_net& nt = a.net;
  const int t = threadIdx.x;
  if constexpr (ENC_ONLY) {
    float* X = fa_lds;                // [16][FA_XP]: obs | latent | 0
    float* HE1 = X + FA_R * FA_XP;    // [16][FA_XP]
    float* MID = HE1 + FA_R * FA_XP;  // priv [16][36], he2 [16][enc_h1 + 4]
    const int r0 = blockIdx.x * FA_R, nrows = min(FA_R, a.n - r0);
    fa_encoder<PRESET, 1>(a, X, HE1, MID, r0, nrows, fa_t);
    const int q4 = a.xs >> 2;  // (xs % 32 == 0: whole float4s of the row)
    for (int e = t; e < nrows * q4; e += FA_THREADS) {
      const int r = e / q4, c = 4 * (e - r * q4);
      *reinterpret_cast<float4*>(a.xa_out + (int64_t)(r0 + r) * a.xs + c) = *reinterpret_cast<const float4*>(X + r * FA_XP + c);
    }
  } else {
    constexpr int NA = HEAD_NA;
    uint8_t* lds = reinterpret_cast<uint8_t*>(fa_lds);
    float* X = fa_lds;                // [32][FA_XP]
    float* HE1 = X + OA_R * FA_XP;    // [32][FA_XP]
    float* MID = HE1 + OA_R * FA_XP;  // priv [32][36], he2 [32][enc_h1 + 4]
    uint16_t* H1 = reinterpret_cast<uint16_t*>(lds);               // planes, ac_h0 / 16 slices
    float* H3 = fa_lds;                                            // [32][OA_H3P]
    uint16_t* XP = reinterpret_cast<uint16_t*>(lds + OA_A_BYTES);  // X planes (xs / 16 slices), then H2 planes
    float* HW = reinterpret_cast<float*>(lds + OA_A_BYTES);        // then the head: [NA | 1][HEAD_W] weight rows,
    float* MU = HW + NA * HEAD_W;                                  // [32][16] mu / log-prob terms (actor),
    float* VP = MU + OA_R * 16;                                    // [32][16] value partials (critic)
    const int grp = blockIdx.x & 1, r0 = (blockIdx.x >> 1) * OA_R, nrows = min(OA_R, a.n - r0);
    const int no = nt.num_obs, np = nt.num_priv;
    const float* w = a.w;
    fa_encoder<PRESET, 2>(a, X, HE1, MID, r0, nrows, fa_t);
    // [obs | latent | 0] rows -> hi / mid / lo plane images (thread: 8 consecutive k of one row)
    {
      const int c8 = a.xs >> 3;
      for (int e = t; e < OA_R * c8; e += OA_THREADS) {
        const int r = e / c8, c = e - r * c8;
        const float4 x0 = *reinterpret_cast<const float4*>(X + r * FA_XP + 8 * c);
        const float4 x1 = *reinterpret_cast<const float4*>(X + r * FA_XP + 8 * c + 4);
        uint32_t hh[4], mm[4], ll[4];
        x6_split2(x0.x, x0.y, hh[0], mm[0], ll[0]);
        x6_split2(x0.z, x0.w, hh[1], mm[1], ll[1]);
        x6_split2(x1.x, x1.y, hh[2], mm[2], ll[2]);
        x6_split2(x1.z, x1.w, hh[3], mm[3], ll[3]);
        uint16_t* p = XP + (c >> 1) * OA_SLICE + x6_off(r, c & 1);
        *reinterpret_cast<uint4*>(p) = make_uint4(hh[0], hh[1], hh[2], hh[3]);
        *reinterpret_cast<uint4*>(p + OA_PLANE) = make_uint4(mm[0], mm[1], mm[2], mm[3]);
        *reinterpret_cast<uint4*>(p + 2 * OA_PLANE) = make_uint4(ll[0], ll[1], ll[2], ll[3]);
      }
    }
    __syncthreads();
    FA_PROF(4)
    // this group's body: [obs | latent] -> ac_h0 -> ac_h1 -> ac_h2 (ELU), X -> H1 -> H2 as planes, H3 as fp32 (one
    // copy of the layer code: the three layers differ in their arguments only)
    const int nx = no + nt.latent;
#pragma unroll 1
    for (int l = 0; l < 3; ++l) {
      OaLayer L;
      if (l == 0)
        L = OaLayer{XP, a.xs, w + nt.w1 + (int64_t)grp * nt.ac_h0 * nx, nx, nx, nt.ac_h0, w + nt.b1 + grp * nt.ac_h0, H1, nullptr};
      else if (l == 1)
        L = OaLayer{H1, nt.ac_h0, w + nt.w2 + (int64_t)grp * nt.ac_h1 * nt.ac_h0, nt.ac_h0, nt.ac_h0, nt.ac_h1,
                    w + nt.b2 + grp * nt.ac_h1, XP, nullptr};
      else
        L = OaLayer{XP, nt.ac_h1, w + nt.w3 + (int64_t)grp * nt.ac_h2 * nt.ac_h1, nt.ac_h1, nt.ac_h1, nt.ac_h2,
                    w + nt.b3 + grp * nt.ac_h2, nullptr, H3};
      if (!((a.vec >> (3 + l)) & 1u)) oa_layer<0>(L);
      else if (L.Kw == L.K) oa_layer<2>(L);
      else oa_layer<1>(L);
      __syncthreads();
      FA_PROF(5 + l)
    }
    // heads, as act_head_kernel's: mu a sequential fmaf over k; the value 16 partial sums over k-sixteenths joined by
    // the pairwise tree.  The actor's workgroup writes actions, mu, sigma and log-prob, the critic's the value
    const int64_t so = (int64_t)a.store_row * a.n;
    if (grp == 0) {
      for (int e = t; e < NA * HEAD_W; e += OA_THREADS) HW[e] = w[nt.w4a + e];
      __syncthreads();
      for (int e = t; e < OA_R * NA; e += OA_THREADS) {
        const int r = e & (OA_R - 1), j = e / OA_R;
        float s = 0.f;
        for (int k = 0; k < HEAD_W; ++k) s = fmaf(H3[r * OA_H3P + k], HW[j * HEAD_W + k], s);
        MU[r * 16 + j] = s + w[nt.b4a + j];
      }
      __syncthreads();
      FA_PROF(8)
      for (int i = t; i < nrows * NA; i += OA_THREADS) {
        const int r = i / NA, j = i - r * NA, g = r0 + r;
        const float m = MU[r * 16 + j], sd = w[nt.std_off + j];
        float act;
        MU[r * 16 + j] = act_draw(a.eps, a.row_offset, a.seed, a.counter, g, j, NA, m, sd, act);
        a.actions[(int64_t)g * NA + j] = act;
        if (a.mu) a.mu[(int64_t)g * NA + j] = m;
        if (a.do_store) {
          const int64_t o = (so + g) * NA + j;
          a.store.actions[o] = act;
          a.store.mu[o] = m;
          a.store.sigma[o] = sd;
        }
      }
      __syncthreads();
      if (t < nrows) {
        const int g = r0 + t;
        float lp = 0.f;
        for (int j = 0; j < NA; ++j) lp += MU[t * 16 + j];
        if (a.logp) a.logp[g] = lp;
        if (a.do_store) a.store.logp[so + g] = lp;
      }
    } else {
      for (int e = t; e < HEAD_W; e += OA_THREADS) HW[e] = w[nt.w4c + e];
      __syncthreads();
      for (int e = t; e < OA_R * 16; e += OA_THREADS) {
        const int r = e & (OA_R - 1), q = e / OA_R;
        float s = 0.f;
        for (int k = q * (HEAD_W / 16); k < (q + 1) * (HEAD_W / 16); ++k) s = fmaf(H3[r * OA_H3P + k], HW[k], s);
        VP[r * 16 + q] = s;
      }
      __syncthreads();
      FA_PROF(8)
      if (t < nrows) {
        const int g = r0 + t;
        float vs[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) vs[q] = VP[t * 16 + q];
#pragma unroll
        for (int wd = 8; wd >= 1; wd /= 2)  // pairwise tree, fixed order
#pragma unroll
          for (int q = 0; q < wd; ++q) vs[q] = vs[2 * q] + vs[2 * q + 1];
        const float v = vs[0] + w[nt.b4c];
        if (a.values) a.values[g] = v;
        if (a.do_store) a.store.values[so + g] = v;
      }
    }
    FA_PROF(9)
    // obs / priv / history rows of this tile into storage row `store_row`: obs and the first 16 history rows by the
    // actor's workgroup, priv and the other history rows by the critic's
    if (a.do_store) {
      const int64_t b = so + r0;
      if (grp == 0) copy_rows<OA_THREADS>(a.obs + (int64_t)r0 * no, no, a.store.obs + b * no, no, nrows, no, t);
      else copy_rows<OA_THREADS>(a.priv + (int64_t)r0 * np, np, a.store.priv + b * np, np, nrows, np, t);
      if (a.hist && a.store.hist) {
        const int hd = a.store.hist_dim, ld = a.store.hist_ld > hd ? a.store.hist_ld : hd;
        const int h0 = grp * (OA_R / 2), hn = min(nrows, h0 + OA_R / 2) - h0;
        if (hn > 0) {
          if (a.hist_shift)
            copy_rows_shift<OA_THREADS>(a.hist_shift + (int64_t)(r0 + h0) * hd, hd, a.store.hist + (b + h0) * ld, ld, hn, hd,
                                        a.hist_slot, t);
          else copy_rows<OA_THREADS>(a.hist + (int64_t)(r0 + h0) * hd, hd, a.store.hist + (b + h0) * ld, ld, hn, hd, t);
        }
      }
    }
    FA_PROF(10)
  }
}

// ---------------------------------------------------------------------------------------------------
// Adaptation head: pred = HD2 W_D3^T + b, MSE against the encoder target (F.mse_loss, mean over B*L),
// dHD2 = dpred W_D3 * elu'(HD2); partials dW_D3 [L][H], db_D3 [L], sum of squared errors.
struct AdaptHeadArgs {
  const float* hd2;  // [B][ldh]
  int ldh;
  const float* tgt;  // [B][ldt]
  int ldt;
  float* dhd2;       // [B][ldh]
  const float *w, *b;
  int B, H, L;       // hidden (32), latent (18)
  float* part;
  int part_len;      // L*H + L + 1
};

// CH / CL: the hidden / latent widths as compile-time constants (the presets' 32 / 18: the dot-product loops unroll
// and their LDS reads issue ahead of the FMA chain, same FMA order), 0 = read from the arguments
template <int CH, int CL>
__global__ __launch_bounds__(HEAD_THREADS) void adapt_head_kernel(AdaptHeadArgs a) {
  // every global load (HD2 tile, weights, the encoder targets) issued up front; the prediction dots spread over
  // (row, output) pairs; per-row squared errors summed in output order (as a sequential loop would)
  const int H = CH ? CH : a.H, L = CL ? CL : a.L;
  __shared__ float HS[HEAD_ROWS][MAX_LAT + 1];
  __shared__ float DP[HEAD_ROWS][MAX_LAT + 1];
  __shared__ float WS[MAX_LAT][MAX_LAT + 1];
  __shared__ float TG[HEAD_ROWS][MAX_LAT + 1];  // targets, then squared errors
  __shared__ float ERR[HEAD_ROWS];
  const int t = threadIdx.x;
  const int r0 = blockIdx.x * HEAD_ROWS;
  const int nrows = min(HEAD_ROWS, a.B - r0);
  for (int i = t; i < HEAD_ROWS * H; i += HEAD_THREADS) {
    const int r = i / H, c = i - r * H;
    HS[r][c] = r < nrows ? a.hd2[(int64_t)(r0 + r) * a.ldh + c] : 0.f;
  }
  for (int i = t; i < L * H; i += HEAD_THREADS) WS[i / H][i % H] = a.w[i];
  for (int i = t; i < HEAD_ROWS * L; i += HEAD_THREADS) {
    const int r = i / L, j = i - r * L;
    TG[r][j] = r < nrows ? a.tgt[(int64_t)(r0 + r) * a.ldt + j] : 0.f;
  }
  __syncthreads();
  const float scale = 2.f / ((float)a.B * (float)L);
  for (int i = t; i < HEAD_ROWS * L; i += HEAD_THREADS) {
    const int r = i / L, j = i - r * L;
    float d = 0.f;
    if (r < nrows) {
      float s = 0.f;
      for (int k = 0; k < H; ++k) s = fmaf(HS[r][k], WS[j][k], s);
      const float pred = s + a.b[j];
      d = pred - TG[r][j];
    }
    TG[r][j] = d * d;
    DP[r][j] = scale * d;
  }
  __syncthreads();
  if (t < HEAD_ROWS) {
    float e = 0.f;
    for (int j = 0; j < L; ++j) e += TG[t][j];
    ERR[t] = e;
  }
  __syncthreads();
  float* P = a.part + (int64_t)blockIdx.x * a.part_len;
  // dHD2 (thread = (row, k) pairs)
  for (int i = t; i < nrows * H; i += HEAD_THREADS) {
    const int r = i / H, k = i - r * H;
    float s = 0.f;
    for (int j = 0; j < L; ++j) s = fmaf(DP[r][j], WS[j][k], s);
    a.dhd2[(int64_t)(r0 + r) * a.ldh + k] = s * delu(HS[r][k]);
  }
  // dW_D3 partial (thread = (j, k)); the specialised form runs over every row of the tile (rows past nrows hold
  // DP = 0 and ERR = 0, so they add exact zeros) so that the row loops unroll
  const int nr = CH ? HEAD_ROWS : nrows;
  for (int i = t; i < L * H; i += HEAD_THREADS) {
    const int j = i / H, k = i - j * H;
    float s = 0.f;
    for (int r = 0; r < nr; ++r) s = fmaf(DP[r][j], HS[r][k], s);
    P[i] = s;
  }
  if (t < L) {
    float s = 0.f;
    for (int r = 0; r < nr; ++r) s += DP[r][t];
    P[L * H + t] = s;
  } else if (t == 64) {
    float s = 0.f;
    for (int r = 0; r < nr; ++r) s += ERR[r];
    P[L * H + L] = s;
  }
}

// ---------------------------------------------------------------------------------------------------
// Segmented reduction of partial slices: dst[i] = scale * sum_p src[p * stride + i] (fixed order).
struct Seg {
  const float* src;
  float* dst;
  int64_t len, stride;
  int parts;
  float scale;
  int lpg;      // log2 of the part groups a workgroup splits the parts into (set by launch_seg)
  int blk0, nblk;  // this segment's workgroups in the packed 1-D grid (set by launch_seg)
};
constexpr int MAX_SEGS = 24;
struct SegList {
  Seg s[MAX_SEGS];
  int n;
};

// dst[i] = scale * sum_q src[q * stride + i].  A 256-thread workgroup covers E = 256 / PG consecutive
// elements with PG part groups: thread (g, e) sums parts g, g + PG, ... (8 loads in flight, coalesced over e),
// then group 0 adds the PG partial sums in group order — a fixed order, so the result is deterministic.
// Few-element / many-part segments (per-workgroup head partials, thin weight gradients) use large PG.
__global__ __launch_bounds__(256) void seg_reduce_kernel(SegList L) {
  int si = 0;
  while (si + 1 < L.n && (int)blockIdx.x >= L.s[si + 1].blk0) ++si;
  const Seg& sg = L.s[si];
  const int lpg = sg.lpg, pg = 1 << lpg, E = 256 >> lpg;
  const int e = threadIdx.x & (E - 1), g = threadIdx.x >> (8 - lpg);
  __shared__ float red[256];
  for (int64_t base = (int64_t)(blockIdx.x - sg.blk0) * E; base < sg.len; base += (int64_t)sg.nblk * E) {
    const int64_t i = base + e;
    float acc = 0.f;
    if (i < sg.len) {
      const float* p = sg.src + i;
      int q = g;
      for (; q + 7 * pg < sg.parts; q += 8 * pg) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(p + (int64_t)(q + u * pg) * sg.stride);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
      }
      for (; q < sg.parts; q += pg) acc += p[(int64_t)q * sg.stride];
    }
    if (pg == 1) {
      if (i < sg.len) sg.dst[i] = acc * sg.scale;
      continue;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    if (g == 0 && i < sg.len) {
      float t = 0.f;
      for (int k = 0; k < pg; ++k) t += red[k * E + e];
      sg.dst[i] = t * sg.scale;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
// clip_grad_norm_ (torch.nn.utils.clip_grad_norm_): sum of squares partials, fp64
constexpr int NORM_BLOCKS = 256;
__global__ void sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ part) {
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double x = g[i];
    s += x * x;
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// adaptive learning rate (ppo.py:110-124), clip coefficient, Adam step size, loss bookkeeping
__global__ void ppo_finalize_kernel(const double* __restrict__ part, int nparts, const float* __restrict__ kl_slot,
                                    float grad_scale, float max_norm, float desired_kl, int adaptive, double bc1,
                                    float inv_B, lrl_ppo_ctrl* ctrl) {
  __shared__ double red[64];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 64) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double tot = 0.0;
  for (int i = 0; i < 64; ++i) tot += red[i];
  const float total_norm = (float)sqrt(tot) * grad_scale;
  float clip = max_norm / (total_norm + 1e-6f);
  clip = fminf(clip, 1.f);
  double lr = ctrl->lr;
  const float kl = kl_slot[0] * grad_scale;
  if (adaptive) {
    const double k = (double)kl;
    if (k > (double)desired_kl * 2.0) lr = fmax(1e-5, lr / 1.5);
    else if (k < (double)desired_kl / 2.0 && k > 0.0) lr = fmin(1e-2, lr * 1.5);
  }
  ctrl->lr = lr;
  ctrl->mb[3] = kl;
  ctrl->clip_scale = clip;
  ctrl->total_norm = total_norm;
  ctrl->step_size = (float)(lr / bc1);
  ctrl->loss_sum[0] += (double)ctrl->mb[0];
  ctrl->loss_sum[1] += (double)ctrl->mb[1];
}

// torch.optim.Adam (foreach, no weight decay / amsgrad):
//   m = lerp(m, g, 1-b1); v = b2 v + (1-b2) g^2; p -= step_size * m / (sqrt(v)/sqrt(bc2) + eps)
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, int64_t n, float grad_scale, const lrl_ppo_ctrl* __restrict__ ctrl,
                            float step_size_host, float one_minus_b1, float b2, float one_minus_b2, float bc2_sqrt,
                            float eps, lrl_ppo_ctrl* acc_ctrl) {
  const float clip = ctrl ? ctrl->clip_scale : 1.f;
  const float step = ctrl ? ctrl->step_size : step_size_host;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float gi = g[i] * grad_scale;
    gi = gi * clip;
    float mi = m[i];
    mi = mi + one_minus_b1 * (gi - mi);
    float vi = v[i] * b2;
    vi = vi + one_minus_b2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = p[i] + (-step) * (mi / denom);
  }
  if (acc_ctrl && blockIdx.x == 0 && threadIdx.x == 0) acc_ctrl->loss_sum[2] += (double)acc_ctrl->mb[2];
}

// ---------------------------------------------------------------------------------------------------
// W[r][0:h) -> Wp[r][0:hp) with zero columns [h, hp): the adaptation module's first layer over history rows
// stored at the padded pitch hp (the k-padding contributes exact zeros)
__global__ void pad_cols_kernel(const float* __restrict__ W, int rows, int h, int hp, float* __restrict__ Wp) {
  const int64_t n = (int64_t)rows * hp;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / hp), c = (int)(i - (int64_t)r * hp);
    Wp[i] = c < h ? W[(int64_t)r * h + c] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------
// host side: the network as a list of linear layers, the workspace plans, the GEMM helper that speaks layers, and the
// forward chains the entry points below are made of

// X = [obs | latent] row pitch: 64 for the blind policies (42 + 18), else rounded up to 16 floats (a height-scan
// policy: 235 + 18 -> 256).  Columns nx..XS-1 are zero.
static int xs_of(const lrl_ppo_net& n) {
  if (n.plain) return (n.num_obs + 15) / 16 * 16;  // X = [obs | 0-pad] (14 -> 16)
  const int nx = n.num_obs + n.latent;
  return nx <= 64 ? 64 : (nx + 15) / 16 * 16;
}
constexpr int LATS = 32;    // latent-wide buffers pitch
constexpr int HD2S = 32;    // adaptation hidden-2 pitch
static int hist_pad(int h) { return (h + 15) / 16 * 16; }

// The weight products that run on the x6p kernel (pre-split B, csrc/lrl_gemm.hip): their planes are split from the
// current parameters at the start of each call (one launch).
// main: forward W1 (k padded to X's pitch), W2, W3, the encoder's W2; backward-data W2^T, W3^T, encoder W2^T (the
// rollout act takes the forward ones, PL_W1 .. PL_E2)
enum MainPlane { PL_W1, PL_W2, PL_W3, PL_E2, PL_W2T, PL_W3T, PL_E2T, PL_MAIN };
constexpr int PL_FWD = PL_E2 + 1;
// adaptation: forward Wd1 (k padded to the history pitch), the encoder-target W2, backward-data Wd2^T
enum AdaptPlane { PL_D1, PL_AE2, PL_D2T, PL_ADAPT };

// One linear layer y = x W^T + b, `groups` independent problems side by side: group g reads the input's columns from
// g * in, writes the output's from g * out, and its weights / biases lie out * ldw / out floats behind the previous.
struct Layer {
  int64_t w, b;  // offsets of W [groups][out][ldw] and b [groups][out] in the parameter (and gradient) buffer
  int out, in;   // per group
  int64_t ldw;   // row pitch of W
  int kf;        // the forward's k extent: `in`, or the input's zero-padded width
  int groups;
  int fwd, bwd;  // the plane images of W / W^T among the chain's plane jobs (MainPlane, AdaptPlane), -1: none
};
static Layer layer(int64_t w, int64_t b, int out, int in, int groups = 1, int fwd = -1, int bwd = -1) {
  return Layer{w, b, out, in, in, in, groups, fwd, bwd};
}
struct Net {
  Layer enc[3];   // env-factor encoder, priv -> latent
  Layer body[3];  // [actor; critic] bodies over X = [obs | latent], grouped (actor_only: the actor's half, one group)
  Layer ad[3];    // adaptation module, history -> latent
  Layer tgt[3];   // the encoder as the adaptation's target: its W2 planes are the adaptation set's
  Layer mean;     // the actor's head as a layer (the student act)
  Layer dlat;     // body 1 over X's latent columns alone: its backward-data product is the latent's gradient
};
static Net layers_of(const lrl_ppo_net& n, bool actor_only = false) {
  Net L{};
  const int g = actor_only ? 1 : 2;
  // body 1's k runs over all XS columns of X: columns nx..XS-1 are zero, so the extra products (with the next row's
  // first weights, or the first biases after the last row — finite values; zero planes on the x6p path) add exactly 0,
  // and the product takes the unguarded float4 path
  L.body[0] = layer(n.w1, n.b1, g * n.ac_h0, n.num_obs + n.latent, 1, PL_W1);
  L.body[0].kf = xs_of(n);
  L.body[1] = layer(n.w2, n.b2, n.ac_h1, n.ac_h0, g, PL_W2, PL_W2T);
  L.body[2] = layer(n.w3, n.b3, n.ac_h2, n.ac_h1, g, PL_W3, PL_W3T);
  L.mean = layer(n.w4a, n.b4a, n.num_actions, n.ac_h2);
  if (n.plain) return L;  // no encoder, latent or adaptation module
  L.enc[0] = layer(n.e1w, n.e1b, n.enc_h0, n.num_priv);
  L.enc[1] = layer(n.e2w, n.e2b, n.enc_h1, n.enc_h0, 1, PL_E2, PL_E2T);
  L.enc[2] = layer(n.e3w, n.e3b, n.latent, n.enc_h1);
  for (int i = 0; i < 3; ++i) L.tgt[i] = L.enc[i];
  L.tgt[1].fwd = PL_AE2;
  L.tgt[1].bwd = -1;
  L.ad[0] = layer(n.d1w, n.d1b, n.ad_h0, n.num_hist, 1, PL_D1);
  L.ad[1] = layer(n.d2w, n.d2b, n.ad_h1, n.ad_h0, 1, -1, PL_D2T);
  L.ad[2] = layer(n.d3w, n.d3b, n.latent, n.ad_h1);
  // d latent = dH1 [W1a; W1c][:, num_obs:]  (sum over actor and critic halves: one reduction of length 2*h0)
  L.dlat = L.body[0];
  L.dlat.w += n.num_obs;
  L.dlat.in = n.latent;
  L.dlat.bwd = -1;
  return L;
}

// The planes of one product's B operand as gemm_launch takes it: B [N][K] (NT) or [K][N] (NN) at pitch ldb, group
// g's gb floats on.
static PlaneJob plane_job(const float* B, int64_t ldb, int layout, int N, int K, int groups, int64_t gb) {
  PlaneJob j{};
  j.W = B; j.ldw = ldb; j.gsrc = gb; j.groups = groups; j.trans = layout == GEMM_NN ? 1 : 0;
  j.rows = j.trans ? K : N; j.cols = j.trans ? N : K;
  return j;
}
// a layer's forward and backward-data images, into their slots of j
static void layer_planes(const Layer& l, const float* w, PlaneJob* j) {
  const float* W = w ? w + l.w : nullptr;
  const int64_t gb = l.groups > 1 ? l.out * l.ldw : 0;
  if (l.fwd >= 0) j[l.fwd] = plane_job(W, l.ldw, GEMM_NT, l.out, l.in, l.groups, gb);
  if (l.bwd >= 0) j[l.bwd] = plane_job(W, l.ldw, GEMM_NN, l.in, l.out, l.groups, gb);
}
// lay the jobs' planes one behind the other from base; returns their length in elements
static int64_t place_planes(PlaneJob* j, int n, uint16_t* base) {
  int64_t off = 0;
  for (int i = 0; i < n; ++i) {
    j[i].dst = base ? base + off : nullptr;
    off += (plane_elems(j[i]) + 127) / 128 * 128;
  }
  return off;
}
static int64_t main_plane_jobs(const lrl_ppo_net& n, const float* w, uint16_t* base, PlaneJob (&j)[PL_MAIN]) {
  const Net L = layers_of(n);
  for (auto& l : L.enc) layer_planes(l, w, j);
  for (auto& l : L.body) layer_planes(l, w, j);
  return place_planes(j, PL_MAIN, base);
}
// (the target encoder's weights come from `we`)
static int64_t adapt_plane_jobs(const lrl_ppo_net& n, const float* w, const float* we, uint16_t* base,
                                PlaneJob (&j)[PL_ADAPT]) {
  const Net L = layers_of(n);
  for (auto& l : L.ad) layer_planes(l, w, j);
  for (auto& l : L.tgt) layer_planes(l, we, j);
  return place_planes(j, PL_ADAPT, base);
}

// An activation buffer: rows at a pitch.  In is a read-only one (the caller's inputs).
struct In { const float* p; int64_t ld; };
struct Buf { float* p; int64_t ld; operator In() const { return In{p, ld}; } };
static Buf cols_from(Buf b, int col) { return Buf{b.p ? b.p + col : nullptr, b.ld}; }

// workspace carver: every buffer starts on a 256-byte boundary (base == nullptr: sizes only)
struct Arena {
  char* base;
  int64_t off = 0;
  float* take(int64_t floats) {
    float* r = base ? reinterpret_cast<float*>(base + off) : nullptr;
    off += ((floats * 4 + 255) / 256) * 256;
    return r;
  }
  Buf take(int64_t rows, int64_t ld) { return Buf{take(rows * ld), ld}; }
};

// The workspace of the update and adaptation calls (make_plan), of the rollout act (make_act_plan: the forward
// buffers and the forward planes) and of the student act (make_student_plan); a buffer a form does not have is null.
struct Plan {
  Buf xa, he1, he2, h1, h2, h3, dh3, dh2, dh1, dlat, dhe2, dhe1;
  Buf tgt, hd1, hd2, dhd2, dhd1;
  Buf wd1p;        // adaptation layer-1 weights at the padded history pitch (zero columns past num_hist)
  float* part;     // partial area (reused by phases 1 and 3)
  int64_t part_floats;
  uint16_t* wpl;   // pre-split weight planes (x6p products): the caller's jobs, built once per call
  int64_t bytes;
};

static int64_t splitk_floats(int M, int N, int splits, int groups) { return (int64_t)splits * groups * ((int64_t)M * N + M); }
static int64_t part_floats_of(const Layer& l, int B) {
  return splitk_floats(l.out, l.in, gemm_pick_splits(l.out, l.in, B, l.groups), l.groups);
}

// X, the encoder's hidden layers (not for a plain net) and the bodies' three, `bw` body halves wide
static void take_forward(Arena& a, Plan& p, const lrl_ppo_net& n, int64_t R, int bw) {
  p.xa = a.take(R, xs_of(n));
  if (!n.plain) {
    p.he1 = a.take(R, n.enc_h0);
    p.he2 = a.take(R, n.enc_h1);
  }
  p.h1 = a.take(R, bw * n.ac_h0);
  p.h2 = a.take(R, bw * n.ac_h1);
  p.h3 = a.take(R, bw * n.ac_h2);
}

static Plan make_plan(const lrl_ppo_net& n, int B, char* base) {
  Plan p{};
  Arena a{base};
  const Net L = layers_of(n);
  take_forward(a, p, n, B, 2);
  p.dh3 = a.take(B, 2 * n.ac_h2);
  p.dh2 = a.take(B, 2 * n.ac_h1);
  p.dh1 = a.take(B, 2 * n.ac_h0);
  const int hb = (B + HEAD_ROWS - 1) / HEAD_ROWS;
  // (64 * 8 floats of slack: the head's slice and each product's cursor are rounded up to 64 floats)
  int64_t ph1 = part_floats_of(L.body[2], B) + part_floats_of(L.body[1], B) + part_floats_of(L.body[0], B) +
                (int64_t)hb * hp_len(n.num_actions) + 64 * 8;
  int64_t ph3 = 0;
  if (!n.plain) {
    p.dlat = a.take(B, LATS);
    p.dhe2 = a.take(B, n.enc_h1);
    p.dhe1 = a.take(B, n.enc_h0);
    p.tgt = a.take(B, LATS);
    p.hd1 = a.take(B, n.ad_h0);
    p.hd2 = a.take(B, HD2S);
    p.dhd2 = a.take(B, HD2S);
    p.dhd1 = a.take(B, n.ad_h0);
    p.wd1p = a.take(n.ad_h0, hist_pad(n.num_hist));
    ph1 += part_floats_of(L.enc[2], B) + part_floats_of(L.enc[1], B) + part_floats_of(L.enc[0], B);
    ph3 = part_floats_of(L.ad[1], B) + part_floats_of(L.ad[0], B) +
          (int64_t)hb * (n.latent * n.ad_h1 + n.latent + 1) + 64 * 4;
  }
  p.part_floats = std::max(ph1, ph3);
  p.part = a.take(p.part_floats);
  if (!n.plain) {
    PlaneJob m[PL_MAIN], d[PL_ADAPT];
    const int64_t elems = std::max(main_plane_jobs(n, nullptr, nullptr, m), adapt_plane_jobs(n, nullptr, nullptr, nullptr, d));
    p.wpl = reinterpret_cast<uint16_t*>(a.take((elems + 1) / 2));
  }
  p.bytes = a.off;
  return p;
}

// rollout forward workspace: X [n][XS], HE1, HE2, H1 [n][2 h0], H2, H3, the forward weight planes (LRL_ACT_PLANES=1:
// the x6p kernel for the act's weight products)
static Plan make_act_plan(const lrl_ppo_net& n, int rows, char* base) {
  Plan p{};
  Arena a{base};
  take_forward(a, p, n, rows, 2);
  if (!n.plain) {
    PlaneJob j[PL_MAIN];
    main_plane_jobs(n, nullptr, nullptr, j);
    p.wpl = reinterpret_cast<uint16_t*>(a.take((place_planes(j, PL_FWD, nullptr) + 1) / 2));
  }
  p.bytes = a.off;
  return p;
}

// student act: X, the adaptation module's hidden layers, the actor's half of the bodies, the padded Wd1
static Plan make_student_plan(const lrl_ppo_net& n, int rows, char* base) {
  Plan p{};
  Arena a{base};
  p.xa = a.take(rows, xs_of(n));
  p.hd1 = a.take(rows, n.ad_h0);
  p.hd2 = a.take(rows, HD2S);
  p.h1 = a.take(rows, n.ac_h0);
  p.h2 = a.take(rows, n.ac_h1);
  p.h3 = a.take(rows, n.ac_h2);
  p.wd1p = a.take(n.ad_h0, hist_pad(n.num_hist));
  p.bytes = a.off;
  return p;
}

static int check_net(const lrl_ppo_net* n) {
  if (!n) return lrl_set_error(LRL_E_INVALID, "lrl_ppo: null net");
  if (n->ac_h2 != HEAD_W) return lrl_set_error(LRL_E_INVALID, "lrl_ppo: last actor/critic hidden width must be 128");
  if ((n->activation != 0 && n->activation != 1) || (n->plain != 0 && n->plain != 1))
    return lrl_set_error(LRL_E_INVALID, "lrl_ppo: activation / plain must be 0 or 1");
  if (n->plain) {  // plain MLP bodies over the observations (the navigation policy): tanh, 3 or 12 actions
    if (n->activation != 1) return lrl_set_error(LRL_E_INVALID, "lrl_ppo: a plain net must use tanh (activation = 1)");
    if (n->num_actions != 3 && n->num_actions != HEAD_NA)
      return lrl_set_error(LRL_E_INVALID, "lrl_ppo: a plain net's num_actions must be 3 or 12");
    if (n->latent || n->enc_h0 || n->enc_h1 || n->ad_h0 || n->ad_h1 || n->adapt_begin != n->adapt_end)
      return lrl_set_error(LRL_E_INVALID, "lrl_ppo: a plain net has no encoder, latent or adaptation module");
    if (n->num_obs <= 0 || n->ac_h0 <= 0 || n->ac_h1 <= 0)
      return lrl_set_error(LRL_E_INVALID, "lrl_ppo: a plain net needs num_obs, ac_h0, ac_h1 > 0");
    return 0;
  }
  if (n->activation != 0)
    return lrl_set_error(LRL_E_INVALID, "lrl_ppo: tanh is implemented for plain nets only (activation = 1 needs plain = 1)");
  if (n->num_actions != HEAD_NA) return lrl_set_error(LRL_E_INVALID, "lrl_ppo: num_actions must be 12");
  if (n->latent > MAX_LAT || n->ad_h1 > MAX_LAT) return lrl_set_error(LRL_E_INVALID, "lrl_ppo: latent/adaptation widths > 32");
  return 0;
}

// Optional timing of the update's largest product (the actor/critic layer-2 weight gradient, 2 x 256x512
// over the minibatch rows): HIP events around that launch on its stream, read back by lrl_ppo_timing.
struct GemmTimer {
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  size_t used = 0;
};
static GemmTimer g_timer;
static hipEvent_t timer_event() {
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}
static void timer_begin(hipStream_t st) {
  if (!g_timer.on) return;
  if (g_timer.used == g_timer.ev.size()) g_timer.ev.emplace_back(timer_event(), timer_event());
  auto& pr = g_timer.ev[g_timer.used];
  if (pr.first) (void)hipEventRecord(pr.first, st);
}
static void timer_end(hipStream_t st) {
  if (!g_timer.on) return;
  auto& pr = g_timer.ev[g_timer.used++];
  if (pr.second) (void)hipEventRecord(pr.second, st);
}

// A weight gradient dW[g][m][n] = sum_k dY[k][m] X[rows(k)][n] as a split-k product and its reduction: partials
// [split][group][M][N] at `part`, the bias gradient's [split][group][M] (column sums of dY) behind them, one segment
// each into dw and db.  Group g's operands start gy / gx floats on; splits == 0: gemm_pick_splits' count.
struct SplitK { GemmP p; Seg s[2]; };  // (weights' segment, biases')
// False, and nothing set, when the partials would pass `end`; else `part` moves behind them.
static bool splitk_job(int M, int N, int K, int groups, int splits, In dY, int64_t gy, In X, int64_t gx,
                       const int64_t* rows, float* dw, float* db, float*& part, const float* end, SplitK& o) {
  if (!splits) splits = gemm_pick_splits(M, N, K, groups);
  const int64_t gmn = (int64_t)groups * M * N, gm = (int64_t)groups * M;
  if (splitk_floats(M, N, splits, groups) > end - part) return false;
  GemmP p{};
  p.A = dY.p; p.lda = dY.ld; p.ga = gy; p.B = X.p; p.ldb = X.ld; p.gb = gx; p.b_rows = rows;
  p.M = M; p.N = N; p.K = K; p.splits = splits; p.kps = (K + splits - 1) / splits;
  p.gc = (int64_t)M * N; p.ldc = N; p.part_stride = gmn;
  p.C = part;
  p.bias_part = part + splits * gmn;
  o.p = p;
  o.s[0] = Seg{part, dw, gmn, gmn, splits, 1.f};
  o.s[1] = Seg{p.bias_part, db, gm, gm, splits, 1.f};
  part = p.bias_part + splits * gm;
  return true;
}

// The products of a call, layer by layer: launched on `st` as they are named, or, after collect(), appended to the
// caller's job list (as gemm_launch would receive them) for it to launch alone or packed (launch_jobs); everything
// else the helpers do stays the same.
struct G {
  hipStream_t st;
  const float* w;  // the parameters the layers' offsets point into
  int m;           // rows of every product's batch dimension
  float* part = nullptr;      // cursor in the partial area: the next weight gradient's partials
  float* part_end = nullptr;  // its end: a product that would not fit is refused before launch
  int rc = 0;
  const PlaneJob* planes = nullptr;  // the chain's plane jobs: a layer with an image there runs on it
  bool tanh_act = false;             // the activation epilogues: tanh / 1 - y^2 instead of ELU / elu'
  GemmJob* jobs = nullptr;
  int njobs = 0, max_jobs = 0;
  void with(const PlaneJob* chain) { planes = chain; }
  void collect(GemmJob* list, int first, int max) { jobs = list; njobs = first; max_jobs = max; }  // next: list[first]
  void launch(GemmP& p, int image, int layout, int epi, int groups) {
    if (planes && image >= 0) gemm_use_planes(p, planes[image]);
    if (!jobs) rc = gemm_launch(p, layout, epi, groups, st);
    else if (njobs < max_jobs) jobs[njobs++] = GemmJob{p, layout, epi, groups};
    else rc = LRL_E_INVALID;
  }
  // y = act(x[rows] W^T + b); W read from `Wsub` where given (a re-pitched copy) instead of the parameters
  void forward(const Layer& l, In x, const int64_t* rows, Buf y, bool act, const float* Wsub = nullptr) {
    if (rc) return;
    GemmP p{};
    p.A = x.p; p.lda = x.ld; p.a_rows = rows; p.B = Wsub ? Wsub : w + l.w; p.ldb = l.ldw; p.C = y.p; p.ldc = y.ld;
    p.bias = w + l.b;
    p.M = m; p.N = l.out; p.K = l.kf; p.splits = 1;
    if (l.groups > 1) { p.ga = l.in; p.gb = l.out * l.ldw; p.gc = l.out; p.gbias = l.out; }
    launch(p, l.fwd, GEMM_NT, act ? (tanh_act ? EPI_BIAS_TANH : EPI_BIAS_ELU) : EPI_BIAS, l.groups);
  }
  // dX = dY W (* act'(aux) where aux, the layer's activated input, is given)
  void backward_data(const Layer& l, In dY, Buf dX, In aux) {
    if (rc) return;
    GemmP p{};
    p.A = dY.p; p.lda = dY.ld; p.B = w + l.w; p.ldb = l.ldw; p.C = dX.p; p.ldc = dX.ld; p.aux = aux.p; p.ld_aux = aux.ld;
    p.M = m; p.N = l.in; p.K = l.out; p.splits = 1;
    if (l.groups > 1) { p.ga = l.out; p.gb = l.out * l.ldw; p.gc = l.in; p.gaux = l.in; }
    launch(p, l.bwd, GEMM_NN, aux.p ? (tanh_act ? EPI_DTANH : EPI_DELU) : EPI_STORE, l.groups);
  }
  // partial dW[o][i] = sum_b dY[b][o] X[rows(b)][i] at the cursor; its segments (weights then biases) go to L
  void weight_grad(const Layer& l, In dY, In X, const int64_t* rows, float* grads, SegList& L) {
    if (rc) return;
    const bool grouped = l.groups > 1;
    SplitK k;
    if (L.n + 2 > MAX_SEGS || !splitk_job(l.out, l.in, m, l.groups, 0, dY, grouped ? l.out : 0, X, grouped ? l.in : 0,
                                          rows, grads + l.w, grads + l.b, part, part_end, k)) {
      rc = LRL_E_INVALID;
      return;
    }
    launch(k.p, -1, GEMM_TN, EPI_PARTIAL, l.groups);
    if (rc) return;
    L.s[L.n++] = k.s[0];
    L.s[L.n++] = k.s[1];
    part = reinterpret_cast<float*>(((reinterpret_cast<uintptr_t>(part) + 255) / 256) * 256);
  }
};

// Launch the collected jobs all[idx[0 .. n)] in that order: as one multi-problem launch where the set is one that
// gemm_launch_multi offers, one by one otherwise (other widths, the fp32 paths of lrl_debug_gemm_paths, LRL_GEMM_X6=0).
static int launch_jobs(const GemmJob* all, const int* idx, int n, hipStream_t st) {
  GemmJob js[MAX_MULTI_JOBS];
  if (n > MAX_MULTI_JOBS) return LRL_E_INVALID;
  for (int i = 0; i < n; ++i) js[i] = all[idx[i]];
  if (n > 1) {
    const int r = gemm_launch_multi(js, n, st);
    if (r) return r < 0 ? r : 0;
  }
  for (int i = 0; i < n; ++i)
    if (int rc = gemm_launch(js[i].p, js[i].layout, js[i].epi, js[i].groups, st)) return rc;
  return 0;
}

// How the backward tail of lrl_ppo_forward_backward launches its eight products, LRL_PPO_BWD_MULTI read at every call
// (a test flips it in one process): 1 (default) = three multi-problem launches on the caller's stream, the encoder's
// products riding in front of the weight gradients' workgroups — {dWe3, dhe2 | dW3}, {dWe2, dhe1 | dW1}, {dWe1 | dW2};
// 2 and 3 = the same riders on other hosts (measurement switches: dW3, dW2, dW1 and dW2, dW1, dW3); 0 = eight
// launches, the encoder's chain forked to the library's second stream (below).  Every setting gives the same bits.
static int bwd_multi_mode() {
  const char* e = getenv("LRL_PPO_BWD_MULTI");
  return e && e[0] >= '0' && e[0] <= '3' ? e[0] - '0' : 1;
}

// The fallback path (LRL_PPO_BWD_MULTI=0; the default packs the chain into the weight-gradient launches instead): the
// env-factor encoder's backward chain (five small products at the minibatch's rows, latency-bound) runs on a
// second stream of the library's own, beside the actor / critic weight gradients of the same minibatch (they share no
// buffer: the chain reads dlat / he1 / he2 / priv and the weights, writes dhe1 / dhe2 and its own partial slices).
// One stream and two events per device, created on first use.  LRL_PPO_FORK=0 (read at every call) keeps everything on
// the caller's stream.
struct Fork {
  hipStream_t st = nullptr;
  hipEvent_t go = nullptr, done = nullptr;
};
// The fork lives on the device of the caller's stream (hipStreamGetDevice; the null stream means the current device),
// and each device's fork is created once under a mutex, so concurrent first calls do not race.  Host threads sharing a
// device share its fork: the stream is in order, so a later `done` record still covers an earlier caller's chain (at
// worst a caller waits for more work than its own).
static Fork* fork_for_device(hipStream_t caller) {
  const char* e = getenv("LRL_PPO_FORK");
  if (e && e[0] == '0') return nullptr;
  static Fork forks[64];
  static std::mutex mu;
  int dev = 0;
  if (caller) {
    hipDevice_t d = 0;
    if (hipStreamGetDevice(caller, &d) != hipSuccess) return nullptr;
    dev = (int)d;
  } else if (hipGetDevice(&dev) != hipSuccess) {
    return nullptr;
  }
  if (dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  Fork& f = forks[dev];
  if (!f.st) {
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return nullptr;
    const bool sw = cur != dev;  // stream and events are created on the caller's device
    if (sw && hipSetDevice(dev) != hipSuccess) return nullptr;
    Fork nf;
    const bool ok = hipStreamCreateWithFlags(&nf.st, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&nf.go, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&nf.done, hipEventDisableTiming) == hipSuccess;
    if (sw) (void)hipSetDevice(cur);
    if (!ok) return nullptr;
    f = nf;
  }
  return &f;
}

static void launch_seg(const SegList& L0, hipStream_t st) {
  SegList L = L0;
  int total = 0;
  for (int i = 0; i < L.n; ++i) {
    Seg& s = L.s[i];
    // split the parts over more groups while the segment's grid is small and each group keeps >= 4 parts
    int lpg = 0;
    while (lpg < 6 && (4 << (lpg + 1)) <= s.parts && (s.len << lpg) < 2048 * 256) ++lpg;
    s.lpg = lpg;
    s.nblk = (int)std::min<int64_t>((s.len + (256 >> lpg) - 1) / (256 >> lpg), 2048);
    s.blk0 = total;
    total += s.nblk;
  }
  if (total > 0) hipLaunchKernelGGL(seg_reduce_kernel, dim3(total), dim3(256), 0, st, L);
}

// Split the first n jobs' matrices into their planes where `on` (one launch); else no job of the chain has planes and
// every product reads its fp32 B
template <int NJ>
static int split_planes(PlaneJob (&j)[NJ], int n, bool on, hipStream_t st) {
  if (on) return x6_planes_launch(j, n, st);
  for (auto& q : j) q.dst = nullptr;
  return 0;
}

// ---- the chains ----
// X = [obs[rows] | 0]: the latent's columns are written by the encoder (or the adaptation module) behind it
static void prep_x(const lrl_ppo_net& n, const float* obs, const int64_t* rows, int m, Buf xa, hipStream_t st) {
  hipLaunchKernelGGL(ppo_prep_kernel, dim3(prep_blocks(m, (int)xa.ld)), dim3(256), 0, st, obs, rows, m, n.num_obs,
                     (int)xa.ld, xa.p);
}
// latent = env_factor_encoder(priv[rows])
static void encoder_forward(G& g, const Layer (&e)[3], In priv, const int64_t* rows, const Plan& P, Buf latent) {
  g.forward(e[0], priv, rows, P.he1, true);
  g.forward(e[1], P.he1, nullptr, P.he2, true);
  g.forward(e[2], P.he2, nullptr, latent, false);
}
// H1, H2, H3 of the actor / critic bodies over X
static void body_forward(G& g, const Layer (&b)[3], const Plan& P) {
  g.forward(b[0], P.xa, nullptr, P.h1, true);
  g.forward(b[1], P.h1, nullptr, P.h2, true);
  g.forward(b[2], P.h2, nullptr, P.h3, true);
}
// hd1 = act(hist[rows] Wd1^T + b).  History rows that carry finite padding up to the 16-float pitch (and are float4
// aligned) run k = hpad against zero-padded weights, so the product reads float4 rows
static void adaptation_l1_forward(G& g, Layer l, In hist, const int64_t* rows, const Plan& P) {
  const int h = l.in, hpad = hist_pad(h);
  if (hist.ld >= hpad && hist.ld % 4 == 0 && ((uintptr_t)hist.p & 15) == 0 && hpad != h) {
    const int64_t cnt = (int64_t)l.out * hpad;
    hipLaunchKernelGGL(pad_cols_kernel, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 1024)), dim3(256), 0, g.st,
                       g.w + l.w, l.out, h, hpad, P.wd1p.p);
    l.kf = hpad;
    l.ldw = hpad;
    g.forward(l, hist, rows, P.hd1, true, P.wd1p.p);
  } else {
    l.fwd = -1;
    g.forward(l, hist, rows, P.hd1, true);
  }
}

// The PPO loss head over H3 (dH3 and the per-workgroup partials of the head's gradients, the KL and the two losses)
// and the segments that reduce those partials, from the cursor `part`
static void launch_loss_head(const lrl_ppo_net& n, const float* w, float* grads, const lrl_ppo_batch* bt,
                             const lrl_ppo_hparams* hp, lrl_ppo_ctrl* ctrl, const Plan& P, float*& part, SegList& L,
                             hipStream_t st) {
  const int B = bt->batch, na = n.num_actions, hb = (B + HEAD_ROWS - 1) / HEAD_ROWS;
  HeadArgs ha{};
  ha.h3 = P.h3.p; ha.dh3 = P.dh3.p;
  ha.w4a = w + n.w4a; ha.b4a = w + n.b4a; ha.w4c = w + n.w4c; ha.b4c = w + n.b4c; ha.stdv = w + n.std_off;
  ha.actions = bt->actions; ha.old_mu = bt->mu; ha.old_sigma = bt->sigma; ha.tv = bt->values; ha.ret = bt->returns;
  ha.adv = bt->adv; ha.old_logp = bt->logp; ha.rows = bt->rows;
  ha.B = B; ha.na = na; ha.clip = hp->clip_param; ha.ent_coef = hp->entropy_coef; ha.vcoef = hp->value_loss_coef;
  ha.clipped_value = hp->use_clipped_value_loss;
  ha.part = part; ha.part_len = hp_len(na);
  if (n.plain && na == 3) hipLaunchKernelGGL((ppo_head_kernel<3, true>), dim3(hb), dim3(HEAD_THREADS), 0, st, ha);
  else if (n.plain) hipLaunchKernelGGL((ppo_head_kernel<HEAD_NA, true>), dim3(hb), dim3(HEAD_THREADS), 0, st, ha);
  else hipLaunchKernelGGL((ppo_head_kernel<HEAD_NA, false>), dim3(hb), dim3(HEAD_THREADS), 0, st, ha);
  const int64_t pl = hp_len(na);
  const float invB = 1.f / (float)B;
  L.s[L.n++] = Seg{part + hp_w4a(na), grads + n.w4a, (int64_t)na * HEAD_W, pl, hb, 1.f};
  L.s[L.n++] = Seg{part + hp_b4a(na), grads + n.b4a, na, pl, hb, 1.f};
  L.s[L.n++] = Seg{part + hp_w4c(na), grads + n.w4c, HEAD_W, pl, hb, 1.f};
  L.s[L.n++] = Seg{part + hp_b4c(na), grads + n.b4c, 1, pl, hb, 1.f};
  L.s[L.n++] = Seg{part + hp_std(na), grads + n.std_off, na, pl, hb, 1.f};
  L.s[L.n++] = Seg{part + hp_kl(na), grads + n.kl_slot, 1, pl, hb, invB};
  L.s[L.n++] = Seg{part + hp_kl(na) + 1, &ctrl->mb[1], 1, pl, hb, invB};
  L.s[L.n++] = Seg{part + hp_kl(na) + 2, &ctrl->mb[0], 1, pl, hb, invB};
  part += ((hb * pl + 63) / 64) * 64;
}

}  // namespace lrl

using namespace lrl;

static bool act_planes_on() {
  const char* e = getenv("LRL_ACT_PLANES");  // (read per call: A/B timing in one process)
  return e && e[0] == '1' && gemm_x6p_enabled();
}

// The envelope of act_fused_kernel: of its encoder part (LDS pitches, whole tile runs per wave), which alone writes X
// for the GEMM chain, and with `body` of the whole act (the plane regions of its LDS, whole 32-column tiles and 32-k
// chunks in every body layer).
static bool fused_envelope(const lrl_ppo_net& n, bool body) {
  auto run_ok = [](int Ng) {  // fa_layer: equal runs per wave
    if (Ng % 16) return false;
    const int T = Ng / 16;
    return T < 4 || T % 4 == 0;
  };
  if (!(xs_of(n) % 32 == 0 && xs_of(n) <= 256 && n.num_priv <= 32 && n.enc_h0 <= 256 && n.enc_h0 % 32 == 0 &&
        n.enc_h1 % 32 == 0 && n.enc_h1 + 4 <= FA_ENC_MIDP && n.latent <= 32 && run_ok(n.enc_h0) && run_ok(n.enc_h1)))
    return false;
  auto run8_ok = [](int Ng) { return Ng / 16 < 8 || (Ng / 16) % 8 == 0; };  // its encoder's runs over 8 waves
  return !body || (run8_ok(n.enc_h0) && run8_ok(n.enc_h1) && xs_of(n) <= OA_MAX_XS && n.num_obs + n.latent >= 4 && n.ac_h0 % 32 == 0 && n.ac_h0 <= OA_MAX_H0 &&
                   n.ac_h1 % 32 == 0 && n.ac_h1 <= OA_MAX_H1 && n.ac_h2 == HEAD_W && n.num_actions == HEAD_NA);
}
// LRL_ACT_ENC_FUSED=0: the prep kernel + three GEMM launches instead of the kernel's encoder part (read per call so a
// test can switch it inside one process)
static bool act_enc_fused(const lrl_ppo_net& n) {
  const char* e = getenv("LRL_ACT_ENC_FUSED");
  return !(e && e[0] == '0') && fused_envelope(n, false);
}
// The rows at which the one-launch act is the default (the measured table is in DESIGN.md §9).  The kernel holds one
// workgroup per CU (144 KB of LDS) and a workgroup takes about 58 us whatever the grid, so the launch costs one such
// round per 256 workgroups = 4,096 rows on the MI355X's 256 CUs: above that a second round starts and the chain, whose
// cost grows with the activations alone, is faster; below 2,048 rows the chain's five launches are shorter than one round.
constexpr int ACT_FUSED_MIN_ROWS = 2048, ACT_FUSED_MAX_ROWS = 4096;
// The one-launch act or the GEMM chain (LRL_ACT_FUSED read per call: A/B timing and the tests that compare the two).
// The one-launch act computes what the chain computes where the chain's body products run on gemm_x6_kernel, that is
// from X6_MIN_M rows and with the bf16-split families on: outside that, and outside the kernel's envelope, every
// setting takes the chain.  Inside, LRL_ACT_FUSED=0 takes the chain, =1 the one-launch act, and unset the one-launch
// act from ACT_FUSED_MIN_ROWS to ACT_FUSED_MAX_ROWS rows.
static bool fused_act_fits(const lrl_ppo_net& n, int rows) {
  const char* e = getenv("LRL_ACT_FUSED");
  if (e && e[0] == '0') return false;
  if (rows < X6_MIN_M || !gemm_x6_enabled() || !fused_envelope(n, true)) return false;
  return (e && e[0] == '1') || (rows >= ACT_FUSED_MIN_ROWS && rows <= ACT_FUSED_MAX_ROWS);
}
// Launch act_fused_kernel, whole (`body`) or its encoder part: the float4 bits of the weight rows it reads, and the
// instance specialised for the presets' encoder widths where they and its bits hold.
static void launch_act_fused(FusedActArgs& fa, bool body, hipStream_t st) {
  const lrl_ppo_net& n = fa.net;
  auto al = [&](int64_t off, int ld) { return (reinterpret_cast<uintptr_t>(fa.w + off) & 15) == 0 && ld % 4 == 0; };
  fa.vec = (al(n.e2w, n.enc_h0) ? 2u : 0u) | (al(n.e3w, n.enc_h1) ? 4u : 0u);
  if (body)
    fa.vec |= (al(n.w1, n.num_obs + n.latent) ? 8u : 0u) | (al(n.w2, n.ac_h0) ? 16u : 0u) | (al(n.w3, n.ac_h1) ? 32u : 0u);
  const bool preset = n.enc_h0 == 256 && n.enc_h1 == 128 && n.latent <= 32 && (fa.vec & 6u) == 6u;
  const dim3 block(body ? OA_THREADS : FA_THREADS);
  if (body) {
    const dim3 grid(2 * ((fa.n + OA_R - 1) / OA_R));
    if (preset) hipLaunchKernelGGL(act_fused_kernel<true>, grid, block, OA_LDS_BYTES, st, fa);
    else hipLaunchKernelGGL(act_fused_kernel<false>, grid, block, OA_LDS_BYTES, st, fa);
  } else {
    const dim3 grid((fa.n + FA_R - 1) / FA_R);
    const size_t lds = FA_ENC_LDS_FLOATS * sizeof(float);
    if (preset) hipLaunchKernelGGL((act_fused_kernel<true, true>), grid, block, lds, st, fa);
    else hipLaunchKernelGGL((act_fused_kernel<false, true>), grid, block, lds, st, fa);
  }
}

extern "C" int64_t lrl_ppo_act_workspace_bytes(const lrl_ppo_net* net, int32_t n) {
  if (check_net(net) || n <= 0) return -1;
  return make_act_plan(*net, n, nullptr).bytes;
}

extern "C" int lrl_debug_act_profile(unsigned long long* out, int reset) {
#ifdef LRL_ACT_PROFILE
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_act_prof), sizeof(unsigned long long) * 12) != hipSuccess) return -2;
  if (reset) {
    unsigned long long z[12] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_act_prof), z, sizeof(z)) != hipSuccess) return -2;
  }
  return 12;
#else
  (void)out;
  (void)reset;
  return 0;
#endif
}

// lrl_ppo_act, and lrl_ppo_act_shift with hist_shift (NULL: hist is read only, as lrl_ppo_act)
static int32_t ppo_act(const lrl_ppo_net* net, const float* params, const float* obs, const float* priv,
                       const float* hist, int32_t n, const float* eps, uint64_t seed, uint64_t counter,
                       int64_t row_offset, float* actions, float* mu, float* values, float* logp, const lrl_rollout_store* store,
                       int32_t store_row, void* workspace, void* stream, float* hist_shift, int32_t hist_slot) {
  if (int rc = check_net(net)) return rc;
  if (hist_shift && (hist_shift != hist || !store || !store->hist || hist_slot <= 0 || store->hist_dim % hist_slot != 0))
    return lrl_set_error(LRL_E_INVALID, "lrl_ppo_act_shift: hist_shift must be hist, with a history store and a slot "
                                        "width that divides its hist_dim");
  if (!params || !obs || (!priv && !net->plain) || !actions || !workspace || n <= 0)
    return lrl_set_error(LRL_E_INVALID, "lrl_ppo_act: null argument or n <= 0");
  if (store && (!store->obs || (!store->priv && priv) || !store->actions || !store->values || !store->logp ||
                !store->mu || !store->sigma || store->hist_dim < 0 ||
                (store->hist_ld != 0 && store->hist_ld < store->hist_dim)))
    return lrl_set_error(LRL_E_INVALID, "lrl_ppo_act: incomplete rollout store");
  const lrl_ppo_net& nt = *net;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the call's inputs and outputs, as the head kernel and the fused kernel both take them
  auto io = [&](auto& a) {
    a.obs = obs; a.priv = priv; a.hist = hist; a.eps = eps; a.n = n;
    a.seed = seed; a.counter = counter; a.row_offset = row_offset;
    a.actions = actions; a.mu = mu; a.values = values; a.logp = logp;
    if (store) a.store = *store;
    a.store_row = store_row; a.do_store = store ? 1 : 0;
    a.hist_shift = hist_shift; a.hist_slot = hist_slot;
  };
  // (a plain net — priv / hist may be NULL: they are only copied into the storage row when given — is the same chain
  // with no encoder, no planes and tanh; the fused kernel is built around the presets' encoder and is not taken)
  const bool full = !nt.plain;
  if (full && fused_act_fits(nt, n)) {  // one launch: act_fused_kernel
    static const bool ok = [] {
      auto set = [](const void* f) {
        return hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, OA_LDS_BYTES) == hipSuccess;
      };
      return set(reinterpret_cast<const void*>(act_fused_kernel<true>)) &&
             set(reinterpret_cast<const void*>(act_fused_kernel<false>));
    }();
    if (!ok) return lrl_set_error(LRL_E_HIP, "lrl_ppo_act: fused kernel LDS attribute");
    FusedActArgs fa{};
    fa.w = params; fa.net = nt; fa.xs = xs_of(nt);
    io(fa);
    launch_act_fused(fa, true, st);
    return hipGetLastError() == hipSuccess ? 0 : lrl_set_error(LRL_E_HIP, "lrl_ppo_act: launch failed");
  }
  Plan P = make_act_plan(nt, n, static_cast<char*>(workspace));
  G g{st, params, n};
  g.tanh_act = nt.plain;
  const Net L = layers_of(nt);
  PlaneJob pj[PL_MAIN];
  if (full) {
    main_plane_jobs(nt, params, P.wpl, pj);
    if (int rc = split_planes(pj, PL_FWD, act_planes_on(), st)) return lrl_set_error(rc, "lrl_ppo_act: planes launch failed");
    g.with(pj);
  }
  if (full && act_enc_fused(nt)) {  // X = [obs | encoder(priv) | 0] in one launch (act_fused_kernel<., true>)
    FusedActArgs fa{};
    fa.w = params; fa.net = nt; fa.obs = obs; fa.priv = priv; fa.n = n; fa.xs = (int)P.xa.ld; fa.xa_out = P.xa.p;
    launch_act_fused(fa, false, st);
  } else {
    prep_x(nt, obs, nullptr, n, P.xa, st);
    if (full) encoder_forward(g, L.enc, In{priv, nt.num_priv}, nullptr, P, cols_from(P.xa, nt.num_obs));
  }
  body_forward(g, L.body, P);
  if (g.rc) return lrl_set_error(g.rc, "lrl_ppo_act: GEMM launch failed");
  ActHeadArgs ah{};
  ah.h3 = P.h3.p; ah.w4a = params + nt.w4a; ah.b4a = params + nt.b4a; ah.w4c = params + nt.w4c; ah.b4c = params + nt.b4c;
  ah.stdv = params + nt.std_off; ah.na = nt.num_actions; ah.no = nt.num_obs; ah.np = nt.num_priv;
  io(ah);
  hipLaunchKernelGGL(act_head_kernel, dim3((n + ACT_ROWS - 1) / ACT_ROWS), dim3(HEAD_THREADS), 0, st, ah);
  return hipGetLastError() == hipSuccess ? 0 : lrl_set_error(LRL_E_HIP, "lrl_ppo_act: launch failed");
}

extern "C" int32_t lrl_ppo_act(const lrl_ppo_net* net, const float* params, const float* obs, const float* priv,
                               const float* hist, int32_t n, const float* eps, uint64_t seed, uint64_t counter,
                               int64_t row_offset, float* actions, float* mu, float* values, float* logp, const lrl_rollout_store* store,
                               int32_t store_row, void* workspace, void* stream) {
  return ppo_act(net, params, obs, priv, hist, n, eps, seed, counter, row_offset, actions, mu, values, logp, store, store_row,
                 workspace, stream, nullptr, 0);
}

extern "C" int32_t lrl_ppo_act_shift(const lrl_ppo_net* net, const float* params, const float* obs, const float* priv,
                                     const float* hist, int32_t n, const float* eps, uint64_t seed, uint64_t counter,
                                     int64_t row_offset, float* actions, float* mu, float* values, float* logp,
                                     const lrl_rollout_store* store, int32_t store_row, void* workspace, void* stream,
                                     float* hist_shift, int32_t hist_slot) {
  return ppo_act(net, params, obs, priv, hist, n, eps, seed, counter, row_offset, actions, mu, values, logp, store, store_row,
                 workspace, stream, hist_shift, hist_slot);
}

// ---- student act (actor_critic.py:160-164): latent = adaptation_module(hist), mean = actor_body([obs, latent]) ----
extern "C" int64_t lrl_ppo_act_student_workspace_bytes(const lrl_ppo_net* net, int32_t n) {
  if (check_net(net) || net->plain || n <= 0) return -1;
  return make_student_plan(*net, n, nullptr).bytes;
}

extern "C" int32_t lrl_ppo_act_student(const lrl_ppo_net* net, const float* params, const float* obs,
                                       const float* hist, int32_t hist_ld, int32_t n, float* mean, float* latent,
                                       void* workspace, void* stream) {
  if (int rc = check_net(net)) return rc;
  if (net->plain) return lrl_set_error(LRL_E_INVALID, "lrl_ppo_act_student: a plain net has no adaptation module");
  if (!params || !obs || !hist || !mean || !workspace || n <= 0)
    return lrl_set_error(LRL_E_INVALID, "lrl_ppo_act_student: null argument or n <= 0");
  const lrl_ppo_net& nt = *net;
  const int hld = hist_ld ? hist_ld : nt.num_hist;
  if (hld < nt.num_hist) return lrl_set_error(LRL_E_INVALID, "lrl_ppo_act_student: hist_ld < num_hist");
  Plan P = make_student_plan(nt, n, static_cast<char*>(workspace));
  hipStream_t st = static_cast<hipStream_t>(stream);
  G g{st, params, n};
  const Net L = layers_of(nt, true);  // the actor's half of the grouped layers: rows [0, h) of each weight / bias
  const Buf lat = cols_from(P.xa, nt.num_obs);
  prep_x(nt, obs, nullptr, n, P.xa, st);
  adaptation_l1_forward(g, L.ad[0], In{hist, hld}, nullptr, P);
  g.forward(L.ad[1], P.hd1, nullptr, P.hd2, true);
  g.forward(L.ad[2], P.hd2, nullptr, lat, false);
  body_forward(g, L.body, P);
  g.forward(L.mean, P.h3, nullptr, Buf{mean, nt.num_actions}, false);
  if (g.rc) return lrl_set_error(g.rc, "lrl_ppo_act_student: GEMM launch failed");
  if (latent &&
      hipMemcpy2DAsync(latent, (size_t)nt.latent * 4, lat.p, (size_t)lat.ld * 4, (size_t)nt.latent * 4, n,
                       hipMemcpyDeviceToDevice, st) != hipSuccess)
    return lrl_set_error(LRL_E_HIP, "lrl_ppo_act_student: latent copy failed");
  return hipGetLastError() == hipSuccess ? 0 : lrl_set_error(LRL_E_HIP, "lrl_ppo_act_student: launch failed");
}

extern "C" int64_t lrl_ppo_workspace_bytes(const lrl_ppo_net* net, int32_t batch) {
  if (check_net(net) || batch <= 0) return -1;
  return make_plan(*net, batch, nullptr).bytes;
}

extern "C" int32_t lrl_ppo_forward_backward(const lrl_ppo_net* net, const float* params, float* grads,
                                            const lrl_ppo_batch* bt, const lrl_ppo_hparams* hp, void* workspace,
                                            lrl_ppo_ctrl* ctrl, void* stream) {
  if (int rc = check_net(net)) return rc;
  if (!bt || !hp || !params || !grads || !workspace || !ctrl || bt->batch <= 0)
    return lrl_set_error(LRL_E_INVALID, "lrl_ppo_forward_backward: null argument");
  const lrl_ppo_net& n = *net;
  const int B = bt->batch;
  const bool full = !n.plain;  // a plain net (the navigation policy): no encoder, no planes (fp32 B operands), tanh
  Plan P = make_plan(n, B, static_cast<char*>(workspace));
  hipStream_t st = static_cast<hipStream_t>(stream);
  G g{st, params, B, P.part, P.part + P.part_floats};
  g.tanh_act = n.plain;
  const Net net_l = layers_of(n);
  const Layer(&enc)[3] = net_l.enc;
  const Layer(&body)[3] = net_l.body;
  // ---- forward ----
  PlaneJob pj[PL_MAIN];
  if (full) {
    main_plane_jobs(n, params, P.wpl, pj);
    if (int rc = split_planes(pj, PL_MAIN, gemm_x6p_enabled(), st))
      return lrl_set_error(rc, "lrl_ppo_forward_backward: planes launch failed");
    g.with(pj);
  }
  const In priv{bt->priv, n.num_priv};
  prep_x(n, bt->obs, bt->rows, B, P.xa, st);
  if (full) encoder_forward(g, enc, priv, bt->rows, P, cols_from(P.xa, n.num_obs));
  body_forward(g, body, P);
  if (g.rc) return lrl_set_error(g.rc, "lrl_ppo_forward_backward: forward GEMM launch failed");
  // ---- head ----
  SegList L{};
  launch_loss_head(n, params, grads, bt, hp, ctrl, P, g.part, L, st);
  // ---- backward ----
  // the data-gradient chain first (dH2, dH1, the latent gradient), then the tail: the encoder's chain (it needs dlat ->
  // dhe2 -> dhe1 in turn) and the actor / critic weight gradients (they need none of them), collected in this one order,
  // which is the order of their partials and segments, and launched as the mode says; the split-k reduction waits
  // for all of them
  g.backward_data(body[2], P.dh3, P.dh2, P.h2);
  g.backward_data(body[1], P.dh2, P.dh1, P.h1);
  if (full) g.backward_data(net_l.dlat, P.dh1, P.dlat, In{});
  enum { DWE3, DHE2, DWE2, DHE1, DWE1, DW3, DW2, DW1, NJOBS };
  GemmJob jobs[NJOBS];
  const int first = full ? 0 : DW3;
  g.collect(jobs, first, NJOBS);
  if (full) {
    g.weight_grad(enc[2], P.dlat, P.he2, nullptr, grads, L);
    g.backward_data(enc[2], P.dlat, P.dhe2, P.he2);
    g.weight_grad(enc[1], P.dhe2, P.he1, nullptr, grads, L);
    g.backward_data(enc[1], P.dhe2, P.dhe1, P.he1);
    g.weight_grad(enc[0], P.dhe1, priv, bt->rows, grads, L);
  }
  g.weight_grad(body[2], P.dh3, P.h2, nullptr, grads, L);
  g.weight_grad(body[1], P.dh2, P.h1, nullptr, grads, L);
  g.weight_grad(body[0], P.dh1, P.xa, nullptr, grads, L);
  int rc = g.rc ? g.rc : (g.njobs == NJOBS ? 0 : LRL_E_INVALID);
  if (rc) return lrl_set_error(rc, "lrl_ppo_forward_backward: backward GEMM launch failed");
  // the launches: one per product (mode 0, and a plain net's three), or the mode's three sets.  With the timing hook
  // on, the timed product (dW2: bench.py --full's roofline_update_gemm) goes alone, so its time keeps its meaning:
  // dW1 hosts dW2's rider, and the other two riders go in a launch of their own
  struct Set { int n, i[MAX_MULTI_JOBS]; };
  Set sets[NJOBS];
  int ns = 0;
  const int mode = full ? bwd_multi_mode() : 0;
  if (mode == 0) {
    for (int i = first; i < NJOBS; ++i) sets[ns++] = Set{1, {i}};
  } else if (g_timer.on) {
    sets[ns++] = Set{3, {DWE3, DHE2, DW3}};
    sets[ns++] = Set{2, {DWE2, DHE1}};
    sets[ns++] = Set{1, {DW2}};
    sets[ns++] = Set{2, {DWE1, DW1}};
  } else {
    static const int hosts[3][3] = {{DW3, DW1, DW2}, {DW3, DW2, DW1}, {DW2, DW1, DW3}};
    const int* host = hosts[mode - 1];
    sets[ns++] = Set{3, {DWE3, DHE2, host[0]}};
    sets[ns++] = Set{3, {DWE2, DHE1, host[1]}};
    sets[ns++] = Set{2, {DWE1, host[2]}};
  }
  // (mode 0: the encoder's five on the fork stream, where there is one)
  Fork* fk = mode == 0 && full ? fork_for_device(st) : nullptr;
  if (fk && (hipEventRecord(fk->go, st) != hipSuccess || hipStreamWaitEvent(fk->st, fk->go, 0) != hipSuccess))
    return lrl_set_error(LRL_E_HIP, "lrl_ppo_forward_backward: stream fork failed");
  for (int s = 0; s < ns && !rc; ++s) {
    const int lead = sets[s].i[0];
    const bool timed = full && sets[s].n == 1 && lead == DW2;
    if (timed) timer_begin(st);
    rc = launch_jobs(jobs, sets[s].i, sets[s].n, fk && lead < DW3 ? fk->st : st);
    if (timed) timer_end(st);
    if (fk && lead == DWE1 && hipEventRecord(fk->done, fk->st) != hipSuccess)
      return lrl_set_error(LRL_E_HIP, "lrl_ppo_forward_backward: stream fork failed");
  }
  if (fk && hipStreamWaitEvent(st, fk->done, 0) != hipSuccess)
    return lrl_set_error(LRL_E_HIP, "lrl_ppo_forward_backward: stream join failed");
  if (rc) return lrl_set_error(rc, "lrl_ppo_forward_backward: backward GEMM launch failed");
  launch_seg(L, st);
  return hipGetLastError() == hipSuccess ? 0 : lrl_set_error(LRL_E_HIP, "lrl_ppo_forward_backward: launch failed");
}

extern "C" int32_t lrl_ppo_optimizer_step(const lrl_ppo_net* net, float* params, const float* grads, float* exp_avg,
                                          float* exp_avg_sq, int64_t step, float grad_scale,
                                          const lrl_ppo_hparams* hp, void* workspace, lrl_ppo_ctrl* ctrl,
                                          void* stream) {
  if (int rc = check_net(net)) return rc;
  if (!params || !grads || !exp_avg || !exp_avg_sq || !hp || !workspace || !ctrl || step < 1)
    return lrl_set_error(LRL_E_INVALID, "lrl_ppo_optimizer_step: bad argument");
  const lrl_ppo_net& n = *net;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // norm partials: the first 2 KB of the workspace (phase-1 scratch, dead once its reduction ran)
  double* norm_part = static_cast<double*>(workspace);
  const int64_t len = n.main_end - n.main_begin;
  hipLaunchKernelGGL(sumsq_kernel, dim3(NORM_BLOCKS), dim3(256), 0, st, grads + n.main_begin, len, norm_part);
  const double bc1 = 1.0 - pow((double)hp->beta1, (double)step);
  const double bc2 = 1.0 - pow((double)hp->beta2, (double)step);
  hipLaunchKernelGGL(ppo_finalize_kernel, dim3(1), dim3(64), 0, st, norm_part, NORM_BLOCKS,
                     grads + n.kl_slot, grad_scale, hp->max_grad_norm, hp->desired_kl, hp->adaptive_schedule, bc1,
                     0.f, ctrl);
  const int blocks = (int)std::min<int64_t>((len + 255) / 256, 2048);
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, st, params + n.main_begin, grads + n.main_begin,
                     exp_avg + n.main_begin, exp_avg_sq + n.main_begin, len, grad_scale, ctrl, 0.f,
                     (float)(1.0 - (double)hp->beta1), hp->beta2, (float)(1.0 - (double)hp->beta2), (float)sqrt(bc2),
                     hp->eps, (lrl_ppo_ctrl*)nullptr);
  return hipGetLastError() == hipSuccess ? 0 : lrl_set_error(LRL_E_HIP, "lrl_ppo_optimizer_step: launch failed");
}

extern "C" int32_t lrl_ppo_adaptation_forward_backward(const lrl_ppo_net* net, const float* params,
                                                       const float* enc_params, float* grads, const lrl_ppo_batch* bt,
                                                       void* workspace, lrl_ppo_ctrl* ctrl, void* stream) {
  if (int rc = check_net(net)) return rc;
  if (net->plain)
    return lrl_set_error(LRL_E_INVALID, "lrl_ppo_adaptation_forward_backward: a plain net has no adaptation module");
  if (!bt || !params || !grads || !workspace || !ctrl || bt->batch <= 0)
    return lrl_set_error(LRL_E_INVALID, "lrl_ppo_adaptation_forward_backward: null argument");
  const lrl_ppo_net& n = *net;
  const int B = bt->batch;
  const int hld = bt->hist_ld ? bt->hist_ld : n.num_hist;
  if (hld < n.num_hist) return lrl_set_error(LRL_E_INVALID, "lrl_ppo_adaptation: hist_ld < num_hist");
  Plan P = make_plan(n, B, static_cast<char*>(workspace));
  hipStream_t st = static_cast<hipStream_t>(stream);
  G g{st, params, B, P.part, P.part + P.part_floats};
  const Net net_l = layers_of(n);
  const Layer(&ad)[3] = net_l.ad;
  // target = env_factor_encoder(priv) with the just-updated weights (torch.no_grad, ppo.py:159-160), read from
  // enc_params (a snapshot of them taken right after the optimiser step, so the next step may proceed) or params
  const float* we = enc_params ? enc_params : params;
  PlaneJob pj[PL_ADAPT];
  adapt_plane_jobs(n, params, we, P.wpl, pj);
  if (int rc = split_planes(pj, PL_ADAPT, gemm_x6p_enabled(), st))
    return lrl_set_error(rc, "lrl_ppo_adaptation: planes launch failed");
  g.with(pj);
  g.w = we;
  encoder_forward(g, net_l.tgt, In{bt->priv, n.num_priv}, bt->rows, P, P.tgt);
  g.w = params;
  // prediction = adaptation_module(obs_history)
  const In hist{bt->hist, hld};
  adaptation_l1_forward(g, ad[0], hist, bt->rows, P);
  g.forward(ad[1], P.hd1, nullptr, P.hd2, true);
  if (g.rc) return lrl_set_error(g.rc, "lrl_ppo_adaptation: forward GEMM launch failed");
  SegList L{};
  float*& part = g.part;
  const int hb = (B + HEAD_ROWS - 1) / HEAD_ROWS;
  AdaptHeadArgs aa{};
  aa.hd2 = P.hd2.p; aa.ldh = HD2S; aa.tgt = P.tgt.p; aa.ldt = LATS; aa.dhd2 = P.dhd2.p; aa.w = params + n.d3w;
  aa.b = params + n.d3b;
  aa.B = B; aa.H = n.ad_h1; aa.L = n.latent; aa.part = part; aa.part_len = n.latent * n.ad_h1 + n.latent + 1;
  if (aa.H == 32 && aa.L == 18)
    hipLaunchKernelGGL((adapt_head_kernel<32, 18>), dim3(hb), dim3(HEAD_THREADS), 0, st, aa);
  else
    hipLaunchKernelGGL((adapt_head_kernel<0, 0>), dim3(hb), dim3(HEAD_THREADS), 0, st, aa);
  {
    const int64_t pl = aa.part_len;
    L.s[L.n++] = Seg{part, grads + n.d3w, (int64_t)n.latent * n.ad_h1, pl, hb, 1.f};
    L.s[L.n++] = Seg{part + n.latent * n.ad_h1, grads + n.d3b, n.latent, pl, hb, 1.f};
    L.s[L.n++] = Seg{part + n.latent * n.ad_h1 + n.latent, &ctrl->mb[2], 1, pl, hb,
                     1.f / ((float)B * (float)n.latent)};
    part += ((hb * pl + 63) / 64) * 64;
  }
  g.weight_grad(ad[1], P.dhd2, P.hd1, nullptr, grads, L);
  g.backward_data(ad[1], P.dhd2, P.dhd1, P.hd1);
  g.weight_grad(ad[0], P.dhd1, hist, bt->rows, grads, L);
  if (g.rc) return lrl_set_error(g.rc, "lrl_ppo_adaptation: backward GEMM launch failed");
  launch_seg(L, st);
  return hipGetLastError() == hipSuccess ? 0 : lrl_set_error(LRL_E_HIP, "lrl_ppo_adaptation: launch failed");
}

extern "C" int32_t lrl_ppo_adaptation_step(const lrl_ppo_net* net, float* params, const float* grads, float* exp_avg,
                                           float* exp_avg_sq, int64_t step, double lr, float grad_scale,
                                           const lrl_ppo_hparams* hp, lrl_ppo_ctrl* ctrl, void* stream) {
  if (int rc = check_net(net)) return rc;
  if (net->plain) return lrl_set_error(LRL_E_INVALID, "lrl_ppo_adaptation_step: a plain net has no adaptation module");
  if (!params || !grads || !exp_avg || !exp_avg_sq || !hp || step < 1)
    return lrl_set_error(LRL_E_INVALID, "lrl_ppo_adaptation_step: bad argument");
  const lrl_ppo_net& n = *net;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const double bc1 = 1.0 - pow((double)hp->beta1, (double)step);
  const double bc2 = 1.0 - pow((double)hp->beta2, (double)step);
  const int64_t len = n.adapt_end - n.adapt_begin;
  const int blocks = (int)std::min<int64_t>((len + 255) / 256, 2048);
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, st, params + n.adapt_begin, grads + n.adapt_begin,
                     exp_avg + n.adapt_begin, exp_avg_sq + n.adapt_begin, len, grad_scale,
                     (const lrl_ppo_ctrl*)nullptr, (float)(lr / bc1), (float)(1.0 - (double)hp->beta1), hp->beta2,
                     (float)(1.0 - (double)hp->beta2), (float)sqrt(bc2), hp->eps, ctrl);
  return hipGetLastError() == hipSuccess ? 0 : lrl_set_error(LRL_E_HIP, "lrl_ppo_adaptation_step: launch failed");
}

// ---- GEMM test entry points: one product (lrl_gemm_f32), and the update's grouped / pitched operand forms, alone
// (lrl_gemm_f32_ex) or as a multi-problem launch (lrl_gemm_f32_multi).  A TN product is the update's split-k job
// (splitk_job) in the caller's workspace with its reduction into C (and db = bias); planes are plane_job's. ----
// Split B into planes in the workspace, point p at them: for the x6p kernel (and nothing else) to run the product
static int use_test_planes(GemmP& p, int layout, int groups, float* workspace, int64_t workspace_floats,
                           hipStream_t st) {
  PlaneJob j = plane_job(p.B, p.ldb, layout, p.N, p.K, groups, p.gb);
  j.dst = reinterpret_cast<uint16_t*>(workspace);
  if (!workspace || plane_elems(j) > 2 * workspace_floats)
    return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32(_ex): workspace too small for the planes");
  if (int rc = x6_planes_launch(&j, 1, st)) return lrl_set_error(rc, "lrl_gemm_f32(_ex): planes launch failed");
  gemm_use_planes(p, j);
  return 0;
}

extern "C" int32_t lrl_gemm_f32(int32_t layout, int32_t epi, int32_t M, int32_t N, int32_t K, const float* A,
                                int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, const float* bias,
                                const float* aux, int64_t ld_aux, const int64_t* rows, float* workspace,
                                int64_t workspace_floats, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  if ((epi == EPI_BIAS_TANH && (layout & 0xff) != GEMM_NT) || (epi == EPI_DTANH && (layout & 0xff) != GEMM_NN))
    return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32: epi 5 is an NT epilogue, epi 6 an NN one");
  if (epi == EPI_DTANH && !aux) return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32: epi 6 needs aux");
  if (layout == GEMM_TN) {
    // split-k into the workspace, then reduce into C (C must be [M][N] contiguous: ldc == N)
    if (ldc != N) return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32: TN needs ldc == N");
    int splits = 0;
    if (const char* e = getenv("LRL_GEMM_SPLITS")) splits = std::max(atoi(e), 0);  // development knob (scripts/tn_sweep.py)
    SplitK k;
    float* part = workspace;
    if (!splitk_job(M, N, K, 1, splits, In{A, lda}, 0, In{B, ldb}, 0, rows, C, const_cast<float*>(bias), part,
                    workspace + workspace_floats, k))
      return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32: workspace too small");
    if (int rc = gemm_launch(k.p, GEMM_TN, EPI_PARTIAL, 1, st)) return lrl_set_error(rc, "lrl_gemm_f32: launch failed");
    SegList L{};
    L.s[L.n++] = k.s[0];
    if (bias) L.s[L.n++] = k.s[1];  // bias = db output
    launch_seg(L, st);
    return hipGetLastError() == hipSuccess ? 0 : lrl_set_error(LRL_E_HIP, "lrl_gemm_f32: launch failed");
  }
  GemmP p{};
  p.A = A; p.lda = lda; p.B = B; p.ldb = ldb; p.C = C; p.ldc = ldc; p.bias = bias; p.aux = aux; p.ld_aux = ld_aux;
  p.M = M; p.N = N; p.K = K; p.splits = 1;
  p.a_rows = rows;
  if (layout & 0x100) {  // pre-split B
    layout &= 0xff;
    if (layout != GEMM_NT && layout != GEMM_NN) return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32: planes need NT / NN");
    if (int rc = use_test_planes(p, layout, 1, workspace, workspace_floats, st)) return rc;
    int rc = gemm_launch(p, layout, epi, 1, st);
    if (rc) return lrl_set_error(rc, "lrl_gemm_f32: launch failure");
    return (gemm_last_path() & 0xff) == FAM_X6P
               ? 0
               : lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32: shape not eligible for the x6p kernel");
  }
  int rc = gemm_launch(p, layout, epi, 1, st);
  return rc ? lrl_set_error(rc, "lrl_gemm_f32: bad layout/epilogue or launch failure") : 0;
}

// The product a descriptor names as gemm_launch takes it (planes apart); for a TN product, its reduction in k.s.
static int32_t desc_job(const lrl_gemm_desc* d, GemmJob& job, SplitK& k) {
  if (!d || !d->A || !d->B || !d->C || d->M <= 0 || d->N <= 0 || d->K <= 0 || d->groups <= 0 || d->splits < 0)
    return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_ex: bad argument");
  const int layout = d->layout, epi = d->epi, groups = d->groups, M = d->M, N = d->N, K = d->K;
  if (d->path_out) *d->path_out = 0;
  if (layout == GEMM_TN) {
    if (epi != EPI_PARTIAL || d->planes) return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_ex: TN is epi 4, no planes");
    if (d->ldc != N) return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_ex: TN needs ldc == N");
    if (d->splits) {  // (only an override is judged: the update's own count stands as it is)
      const int kps = ((K + d->splits - 1) / d->splits + 15) / 16 * 16;  // (gemm_launch rounds a split to whole 16-row slices)
      if ((int64_t)(d->splits - 1) * kps >= K) return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_ex: a split would be empty");
    }
    float* part = d->workspace;
    if (!d->workspace || !splitk_job(M, N, K, groups, d->splits, In{d->A, d->lda}, d->ga, In{d->B, d->ldb}, d->gb,
                                     d->rows, d->C, d->bias, part, d->workspace + d->workspace_floats, k))
      return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_ex: workspace too small");
    job =GemmJob{k.p, layout, epi, groups};
    return 0;
  }
  if (layout != GEMM_NT && layout != GEMM_NN) return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_ex: layout is 0, 2 or 3");
  if (d->splits > 1 || epi == EPI_PARTIAL) return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_ex: NT / NN are not split");
  if ((epi == EPI_BIAS_TANH && layout != GEMM_NT) || (epi == EPI_DTANH && layout != GEMM_NN))
    return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_ex: epi 5 is an NT epilogue, epi 6 an NN one");
  if ((epi == EPI_DELU || epi == EPI_DTANH) && !d->aux) return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_ex: epi 3 / 6 need aux");
  if ((epi == EPI_BIAS || epi == EPI_BIAS_ELU || epi == EPI_BIAS_TANH) && !d->bias)
    return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_ex: epi 1 / 2 / 5 need bias");
  GemmP p{};
  p.A = d->A; p.lda = d->lda; p.B = d->B; p.ldb = d->ldb; p.aux = d->aux; p.ld_aux = d->ld_aux;
  p.M = M; p.N = N; p.K = K; p.splits = 1;
  p.ga = d->ga; p.gb = d->gb; p.gaux = d->gaux;
  p.C = d->C; p.ldc = d->ldc; p.gc = d->gc; p.bias = d->bias; p.gbias = d->gbias; p.a_rows = d->rows;
  k.p = p;  // (splits_out = 1)
  job = GemmJob{p, layout, epi, groups};
  return 0;
}
// the reduction of a TN descriptor's partials into its C (and db = bias)
static void desc_reduce(const lrl_gemm_desc* d, const GemmJob& job, const SplitK& k, SegList& L) {
  if (job.layout != GEMM_TN) return;
  L.s[L.n++] = k.s[0];
  if (d->bias) L.s[L.n++] = k.s[1];
}

extern "C" int32_t lrl_gemm_f32_ex(const lrl_gemm_desc* d, void* stream) {
  GemmJob job;
  SplitK k;
  if (int32_t rc = desc_job(d, job, k)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  GemmP& p = job.p;
  const int layout = job.layout, epi = job.epi, groups = job.groups;
  if (layout == GEMM_TN) {
    if (int rc = gemm_launch(p, GEMM_TN, EPI_PARTIAL, groups, st)) return lrl_set_error(rc, "lrl_gemm_f32_ex: launch failed");
    SegList L{};
    desc_reduce(d, job, k, L);
    launch_seg(L, st);
  } else {
    if (d->planes)
      if (int rc = use_test_planes(p, layout, groups, d->workspace, d->workspace_floats, st)) return rc;
    if (int rc = gemm_launch(p, layout, epi, groups, st))
      return lrl_set_error(rc, "lrl_gemm_f32_ex: bad layout/epilogue or launch failure");
    if (d->planes && (gemm_last_path() & 0xff) != FAM_X6P)
      return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_ex: shape not eligible for the x6p kernel");
  }
  if (d->path_out) *d->path_out = gemm_last_path();
  if (d->splits_out) *d->splits_out = k.p.splits;
  return hipGetLastError() == hipSuccess ? 0 : lrl_set_error(LRL_E_HIP, "lrl_gemm_f32_ex: launch failed");
}

// ---- test entry point of the multi-problem launch (gemm_launch_multi) ----
extern "C" int32_t lrl_gemm_f32_multi(const lrl_gemm_desc* d, int32_t n, void* stream) {
  if (!d || n < 2 || n > MAX_MULTI_JOBS) return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_multi: 2 or 3 descriptors");
  hipStream_t st = static_cast<hipStream_t>(stream);
  GemmJob jobs[MAX_MULTI_JOBS];
  SplitK ks[MAX_MULTI_JOBS];
  for (int i = 0; i < n; ++i) {
    if (d[i].planes) return lrl_set_error(LRL_E_INVALID, "lrl_gemm_f32_multi: no planes");
    if (int32_t rc = desc_job(&d[i], jobs[i], ks[i])) return rc;
  }
  const int r = gemm_launch_multi(jobs, n, st);
  if (r < 0) return lrl_set_error(r, "lrl_gemm_f32_multi: launch failed");
  if (r == 0) return 1;  // not one of the sets on offer: nothing was launched
  SegList L{};
  for (int i = 0; i < n; ++i) {
    desc_reduce(&d[i], jobs[i], ks[i], L);
    if (d[i].splits_out) *d[i].splits_out = ks[i].p.splits;
  }
  launch_seg(L, st);
  if (d[n - 1].path_out) *d[n - 1].path_out = gemm_last_path();
  return hipGetLastError() == hipSuccess ? 0 : lrl_set_error(LRL_E_HIP, "lrl_gemm_f32_multi: launch failed");
}

// ---- timing hook of the dominant update product (bench.py roofline) ----
extern "C" int32_t lrl_ppo_timing(int32_t enable, double* total_ms, int64_t* launches) {
  if (total_ms) {
    double t = 0.0;
    for (size_t i = 0; i < g_timer.used; ++i) {
      float ms = 0.f;
      if (hipEventSynchronize(g_timer.ev[i].second) != hipSuccess ||
          hipEventElapsedTime(&ms, g_timer.ev[i].first, g_timer.ev[i].second) != hipSuccess)
        return lrl_set_error(LRL_E_HIP, "lrl_ppo_timing: event query failed");
      t += ms;
    }
    *total_ms = t;
  }
  if (launches) *launches = (int64_t)g_timer.used;
  g_timer.used = 0;
  g_timer.on = enable != 0;
  return 0;
}
