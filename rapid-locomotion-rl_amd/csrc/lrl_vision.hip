// lrl_vision.hip — the depth encoder (include/lrl_vision.h): a fixed three-layer convolution stack over one depth
// image per sample, then two dense layers, with the MSE gradient of the whole network.
//
//   x = depth * input_scale                       [1][H][W]
//   a1 = elu(conv(x;  16 x 1 x 5 x 5, stride 2, pad 2))   [16][H/2][W/2]
//   a2 = elu(conv(a1; 32 x 16 x 3 x 3, stride 2, pad 1))  [32][H/4][W/4]
//   a3 = elu(conv(a2; 32 x 32 x 3 x 3, stride 2, pad 1))  [32][H/8][W/8]   = the F = H W / 2 features, (c, y, x) order
//   h = elu(fc1([a3 | extra])), pred = fc2(h)
//
// The convolution stack is ONE launch in each direction.  A 512-thread workgroup holds one image and its three
// activation maps in LDS (H W (1 + 4 + 2 + 1/2) floats = 30 H W bytes, plus one pad word per channel plane so that the
// planes of consecutive channels start in different banks) and loops over the images the grid does not cover.  The
// arithmetic is fp32 FMA on the VALU in a fixed order (each input channel's taps by kernel row and column from zero,
// then the channels' sums in order: short chains keep the rounding error near torch's blocked sums), so a
// feature row depends on its image and the weights only.  A wave takes (output-channel block, 64-pixel chunk) units;
// the channel block is wave-uniform, so the weights arrive through scalar loads.
//
// The backward launch recomputes the activations of each image in LDS (nothing but the features ever goes to HBM),
// turns each map into its gradient in place (a3 -> g3, a2 -> g2, a1 -> g1: an element's gradient needs the element
// itself only for elu'), and accumulates the weight gradients in registers: every thread owns fixed (co, ci) kernels
// (nine taps each) of conv3 and conv2 and one tap of conv1 for the whole launch.  At the end a workgroup writes one
// partial row; a second launch adds the rows in workgroup order.  No atomics: the result is the same bits every call.
//
// The dense layers run on the GEMM families (lrl_gemm_f32_ex): NT + bias + ELU, NT + bias, NN * elu', TN with the bias
// gradient.  [features | extra] is one pitched row of the workspace, written by the forward launch.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../include/lrl.h"
#include "lrl_gemm.h"

extern "C" int lrl_set_error(int code, const char* msg);  // lrl_capi.cpp

namespace lrl {

namespace {

constexpr int VT = 512;            // threads of a conv-stack workgroup
constexpr int VW = VT / 64;        // its waves
constexpr int C1 = 16, C2 = 32, C3 = 32;
// one workgroup's partial row of the conv gradients, packed: w1, b1, w2, b2, w3, b3
constexpr int PW1 = 0, PB1 = PW1 + C1 * 25, PW2 = PB1 + C1, PB2 = PW2 + C2 * C1 * 9, PW3 = PB2 + C2,
              PB3 = PW3 + C3 * C2 * 9, PCONV = PB3 + C3;
constexpr int PPITCH = (PCONV + 63) / 64 * 64;  // row pitch of the partials (the tail of a row is never written)
static_assert(PCONV == 14304, "conv parameter count");
static_assert(C3 * C2 == 2 * VT && C2 * C1 == VT && C1 * 25 <= VT, "the weight-gradient ownership below");

struct VisionK {
  const float* params;
  const float* images;
  const float* extra;
  const int64_t* rows;
  float* x;           // [batch][ldx]: features, then extra, then zero padding
  float* features;    // optional [batch][F]
  const float* dfeat; // backward: [batch][F]
  float* partials;    // backward: [gridDim.x][PPITCH]
  int64_t c1w, c1b, c2w, c2b, c3w, c3b;
  int64_t ld_extra;
  int H, W, E, F, ldx, batch;
  float scale;
};

// LDS map, in floats: the image, then the three maps, each channel plane one word longer than its pixels
struct Map {
  int H1, W1, H2, W2, H3, W3, n1, n2, n3, s1, s2, s3, o1, o2, o3, total;
};
__host__ __device__ inline Map lds_map(int H, int W) {
  Map m;
  m.H1 = H / 2; m.W1 = W / 2; m.H2 = H / 4; m.W2 = W / 4; m.H3 = H / 8; m.W3 = W / 8;
  m.n1 = m.H1 * m.W1; m.n2 = m.H2 * m.W2; m.n3 = m.H3 * m.W3;
  m.s1 = m.n1 + 1; m.s2 = m.n2 + 1; m.s3 = m.n3 + 1;
  m.o1 = H * W; m.o2 = m.o1 + C1 * m.s1; m.o3 = m.o2 + C2 * m.s2;
  m.total = m.o3 + C3 * m.s3;
  return m;
}

__device__ __forceinline__ float delu(float v, float a) { return a > 0.f ? v : v * (a + 1.f); }

// out[co][oy][ox] = elu(b[co] + sum_ci sum_ky sum_kx in[ci][2 oy + ky - PAD][2 ox + kx - PAD] w[co][ci][ky][kx]), zero
// outside the input.  Unit u of a wave: CB output channels x 64 consecutive output pixels.
template <int CIN, int COUT, int KS, int PAD, int CB>
__device__ __forceinline__ void conv_fwd(const float* in, int in_stride, int Hin, int Win, float* out, int out_stride,
                                         const float* __restrict__ w, const float* __restrict__ b) {
  const int Ho = Hin >> 1, Wo = Win >> 1, npix = Ho * Wo;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int nchunk = (npix + 63) >> 6, units = (COUT / CB) * nchunk;
  for (int u = wave; u < units; u += VW) {
    const int cg = u / nchunk, ch = u - cg * nchunk, co0 = cg * CB;
    const int p = ch * 64 + lane;
    const bool live = p < npix;
    const int pp = live ? p : 0;
    const int oy = pp / Wo, ox = pp - oy * Wo;
    float acc[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = b[co0 + c];
#pragma unroll 1
    for (int ci = 0; ci < CIN; ++ci) {
      const float* ip = in + ci * in_stride;
      const float* wp = w + ((size_t)co0 * CIN + ci) * (KS * KS);
      float part[CB];  // this input channel's taps, summed from zero: short chains, then one add per channel
#pragma unroll
      for (int c = 0; c < CB; ++c) part[c] = 0.f;
#pragma unroll
      for (int ky = 0; ky < KS; ++ky) {
        const int iy = 2 * oy + ky - PAD;
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) {
          const int ix = 2 * ox + kx - PAD;
          float v = 0.f;
          if ((unsigned)iy < (unsigned)Hin && (unsigned)ix < (unsigned)Win) v = ip[iy * Win + ix];
#pragma unroll
          for (int c = 0; c < CB; ++c) part[c] = fmaf(v, wp[(size_t)c * CIN * KS * KS + ky * KS + kx], part[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < CB; ++c) acc[c] += part[c];
    }
    if (live) {
#pragma unroll
      for (int c = 0; c < CB; ++c) out[(co0 + c) * out_stride + p] = elu_f(acc[c]);
    }
  }
}

// Backward-data of a 3 x 3, stride 2, pad 1 layer, in place over the layer's input map a (ELU outputs):
//   a[ci][iy][ix] <- elu'(a[ci][iy][ix]) sum_co sum_{ky, kx} g[co][(iy + 1 - ky) / 2][(ix + 1 - kx) / 2] w[co][ci][ky][kx]
// over the taps whose (iy + 1 - ky, ix + 1 - kx) are even and inside g.  A unit is CB input channels x one parity
// class of (iy, ix) x 64 pixels of the class, so the taps that count are wave-uniform.
template <int CIN, int COUT, int CB>
__device__ __forceinline__ void conv_bwd_data(float* a, int a_stride, int Hin, int Win, const float* g, int g_stride,
                                              const float* __restrict__ w) {
  const int Ho = Hin >> 1, Wo = Win >> 1, ncls = Ho * Wo;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int nchunk = (ncls + 63) >> 6, units = (CIN / CB) * 4 * nchunk;
  for (int u = wave; u < units; u += VW) {
    const int cg = u / (4 * nchunk), r = u - cg * 4 * nchunk, cls = r / nchunk, ch = r - cls * nchunk;
    const int py = cls >> 1, px = cls & 1, ci0 = cg * CB;
    const int p = ch * 64 + lane;
    const bool live = p < ncls;
    const int pp = live ? p : 0;
    const int y2 = pp / Wo, x2 = pp - y2 * Wo;
    const int iy = 2 * y2 + py, ix = 2 * x2 + px;
    float acc[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = 0.f;
#pragma unroll 1
    for (int co = 0; co < COUT; ++co) {
      const float* gp = g + co * g_stride;
      const float* wp = w + ((size_t)co * CIN + ci0) * 9;
      float part[CB];  // (this output channel's taps from zero, as conv_fwd sums an input channel's)
#pragma unroll
      for (int c = 0; c < CB; ++c) part[c] = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        if ((py + 1 - ky) & 1) continue;  // (wave-uniform)
        const int oy = (iy + 1 - ky) >> 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          if ((px + 1 - kx) & 1) continue;
          const int ox = (ix + 1 - kx) >> 1;
          float v = 0.f;
          if ((unsigned)oy < (unsigned)Ho && (unsigned)ox < (unsigned)Wo) v = gp[oy * Wo + ox];
#pragma unroll
          for (int c = 0; c < CB; ++c) part[c] = fmaf(v, wp[c * 9 + ky * 3 + kx], part[c]);
        }
      }
#pragma unroll
      for (int c = 0; c < CB; ++c) acc[c] += part[c];
    }
    if (live) {
#pragma unroll
      for (int c = 0; c < CB; ++c) {
        float* e = a + (ci0 + c) * a_stride + iy * Win + ix;
        *e = delu(acc[c], *e);
      }
    }
  }
}

// acc[ky][kx] += sum_{oy, ox} g[oy][ox] in[2 oy + ky - 1][2 ox + kx - 1]: one (co, ci) kernel of a 3 x 3 layer.  Three
// levels of short chains: an output row from zero, the rows of the image from zero, then the image onto acc.
__device__ __forceinline__ void conv_dw9(const float* ip, int Hin, int Win, const float* gp, float (&total)[9]) {
  const int Ho = Hin >> 1, Wo = Win >> 1;
  float image[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) image[i] = 0.f;
#pragma unroll 1
  for (int oy = 0; oy < Ho; ++oy) {
    float acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.f;
#pragma unroll 1
    for (int ox = 0; ox < Wo; ++ox) {
      const float gv = gp[oy * Wo + ox];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy + ky - 1;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const int ix = 2 * ox + kx - 1;
          float v = 0.f;
          if ((unsigned)iy < (unsigned)Hin && (unsigned)ix < (unsigned)Win) v = ip[iy * Win + ix];
          acc[ky * 3 + kx] = fmaf(gv, v, acc[ky * 3 + kx]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) image[i] += acc[i];
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) total[i] += image[i];
}

// a bias gradient: the plane's sum (in fp64: one thread per channel adds up to 768 values) onto acc
__device__ __forceinline__ double plane_sum(const float* gp, int n, double acc) {
#pragma unroll 1
  for (int i = 0; i < n; ++i) acc += (double)gp[i];
  return acc;
}

__device__ __forceinline__ void load_image(const VisionK& k, int64_t row, float* img) {
  const float* src = k.images + row * (int64_t)(k.H * k.W);
  for (int i = threadIdx.x; i < k.H * k.W; i += VT) img[i] = src[i] * k.scale;
}

__device__ __forceinline__ void conv_stack(const VisionK& k, const Map& m, float* lds) {
  const float* P = k.params;
  conv_fwd<1, C1, 5, 2, 8>(lds, 0, k.H, k.W, lds + m.o1, m.s1, P + k.c1w, P + k.c1b);
  __syncthreads();
  conv_fwd<C1, C2, 3, 1, 4>(lds + m.o1, m.s1, m.H1, m.W1, lds + m.o2, m.s2, P + k.c2w, P + k.c2b);
  __syncthreads();
  conv_fwd<C2, C3, 3, 1, 4>(lds + m.o2, m.s2, m.H2, m.W2, lds + m.o3, m.s3, P + k.c3w, P + k.c3b);
  __syncthreads();
}

}  // namespace

__global__ __launch_bounds__(VT) void vision_fwd_kernel(VisionK k) {
  extern __shared__ float lds[];
  const Map m = lds_map(k.H, k.W);
  for (int n = blockIdx.x; n < k.batch; n += gridDim.x) {
    const int64_t row = k.rows ? k.rows[n] : n;
    load_image(k, row, lds);
    __syncthreads();
    conv_stack(k, m, lds);
    float* xr = k.x + (int64_t)n * k.ldx;
    for (int f = threadIdx.x; f < k.F; f += VT) {
      const int c = f / m.n3, p = f - c * m.n3;
      const float v = lds[m.o3 + c * m.s3 + p];
      xr[f] = v;
      if (k.features) k.features[(int64_t)n * k.F + f] = v;
    }
    for (int e = threadIdx.x; e < k.ldx - k.F; e += VT) xr[k.F + e] = e < k.E ? k.extra[row * k.ld_extra + e] : 0.f;
    __syncthreads();  // (the next image overwrites the maps)
  }
}

__global__ __launch_bounds__(VT) void vision_bwd_kernel(VisionK k) {
  extern __shared__ float lds[];
  const Map m = lds_map(k.H, k.W);
  const int t = threadIdx.x;
  const float* P = k.params;
  // this thread's weight gradients, summed over the workgroup's images: conv3 kernels t and t + VT, conv2 kernel t,
  // conv1 tap t (t < 400), one bias (t < 16: conv1's, 64 <= t < 96: conv2's, 128 <= t < 160: conv3's)
  float w3a[9], w3b[9], w2[9], w1 = 0.f;
  double bs = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) w3a[i] = w3b[i] = w2[i] = 0.f;
  float* a1 = lds + m.o1;
  float* a2 = lds + m.o2;
  float* a3 = lds + m.o3;
  for (int n = blockIdx.x; n < k.batch; n += gridDim.x) {
    const int64_t row = k.rows ? k.rows[n] : n;
    load_image(k, row, lds);
    __syncthreads();
    conv_stack(k, m, lds);
    const float* dr = k.dfeat + (int64_t)n * k.F;
    for (int f = t; f < k.F; f += VT) {
      const int c = f / m.n3, p = f - c * m.n3;
      float* e = a3 + c * m.s3 + p;
      *e = delu(dr[f], *e);
    }
    __syncthreads();
    // conv3: weights from (a2, g3), then g2 over a2
    conv_dw9(a2 + (t % C2) * m.s2, m.H2, m.W2, a3 + (t / C2) * m.s3, w3a);
    conv_dw9(a2 + (t % C2) * m.s2, m.H2, m.W2, a3 + ((t + VT) / C2) * m.s3, w3b);
    if (t >= 128 && t < 128 + C3) bs = plane_sum(a3 + (t - 128) * m.s3, m.n3, bs);
    __syncthreads();
    conv_bwd_data<C2, C3, 4>(a2, m.s2, m.H2, m.W2, a3, m.s3, P + k.c3w);
    __syncthreads();
    // conv2: weights from (a1, g2), then g1 over a1
    conv_dw9(a1 + (t % C1) * m.s1, m.H1, m.W1, a2 + (t / C1) * m.s2, w2);
    if (t >= 64 && t < 64 + C2) bs = plane_sum(a2 + (t - 64) * m.s2, m.n2, bs);
    __syncthreads();
    conv_bwd_data<C1, C2, 4>(a1, m.s1, m.H1, m.W1, a2, m.s2, P + k.c2w);
    __syncthreads();
    // conv1: one tap per thread from (image, g1)
    if (t < C1 * 25) {
      const int co = t / 25, tap = t - co * 25, ky = tap / 5, kx = tap - ky * 5;
      const float* gp = a1 + co * m.s1;
      float image = 0.f;  // (row, image, launch: the three levels of conv_dw9)
#pragma unroll 1
      for (int oy = 0; oy < m.H1; ++oy) {
        const int iy = 2 * oy + ky - 2;
        if ((unsigned)iy >= (unsigned)k.H) continue;
        float acc = 0.f;
#pragma unroll 1
        for (int ox = 0; ox < m.W1; ++ox) {
          const int ix = 2 * ox + kx - 2;
          if ((unsigned)ix < (unsigned)k.W) acc = fmaf(gp[oy * m.W1 + ox], lds[iy * k.W + ix], acc);
        }
        image += acc;
      }
      w1 += image;
    }
    if (t < C1) bs = plane_sum(a1 + t * m.s1, m.n1, bs);
    __syncthreads();
  }
  float* pr = k.partials + (int64_t)blockIdx.x * PPITCH;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    pr[PW3 + t * 9 + i] = w3a[i];
    pr[PW3 + (t + VT) * 9 + i] = w3b[i];
    pr[PW2 + t * 9 + i] = w2[i];
  }
  if (t < C1 * 25) pr[PW1 + t] = w1;
  if (t < C1) pr[PB1 + t] = (float)bs;
  if (t >= 64 && t < 64 + C2) pr[PB2 + t - 64] = (float)bs;
  if (t >= 128 && t < 128 + C3) pr[PB3 + t - 128] = (float)bs;
}

// grads' conv fields = the partial rows added in workgroup order
__global__ __launch_bounds__(256) void vision_reduce_kernel(const float* __restrict__ partials, int nrows, float* grads,
                                                            int64_t c1w, int64_t c1b, int64_t c2w, int64_t c2b,
                                                            int64_t c3w, int64_t c3b) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= PCONV) return;
  double s = 0.0;  // (up to LRL_VISION_MAX_WORKGROUPS rows: added in fp64, rounded once)
  for (int r = 0; r < nrows; ++r) s += (double)partials[(int64_t)r * PPITCH + p];
  int64_t o;
  if (p < PB1) o = c1w + (p - PW1);
  else if (p < PW2) o = c1b + (p - PB1);
  else if (p < PB2) o = c2w + (p - PW2);
  else if (p < PW3) o = c2b + (p - PB2);
  else if (p < PB3) o = c3w + (p - PW3);
  else o = c3b + (p - PB3);
  grads[o] = (float)s;
}

// d_pred = 2 (pred - target) / (batch out); partial[b] = this workgroup's sum of squared differences, as a double
__global__ __launch_bounds__(256) void vision_loss_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                          int64_t ld_target, const int64_t* __restrict__ rows,
                                                          int64_t total, int out, float scale, float* __restrict__ dpred,
                                                          double* __restrict__ partial) {
  __shared__ double red[256];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / out;
    const int c = (int)(i - r * out);
    const int64_t row = rows ? rows[r] : r;
    const float d = pred[i] - target[row * ld_target + c];
    dpred[i] = d * scale;
    s += (double)d * (double)d;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ void vision_loss_finish_kernel(const double* __restrict__ partial, int n, double inv, double* loss) {
  if (threadIdx.x || blockIdx.x) return;
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += partial[i];
  *loss = s * inv;
}

namespace {

int64_t up64(int64_t x) { return (x + 63) / 64 * 64; }

// the workspace, in floats from its start
struct Ws {
  int64_t x, h1, pred, dpred, dh1, dfeat, part, lossp, gemm, gemm_floats, total;
  int grid, loss_grid;
};
Ws ws_layout(const lrl_vision_net& n, int batch) {
  Ws w;
  const int64_t B = batch;
  int64_t o = 0;
  auto take = [&](int64_t floats) { const int64_t at = o; o += up64(floats); return at; };
  w.grid = std::min(batch, LRL_VISION_MAX_WORKGROUPS);
  w.loss_grid = (int)std::min<int64_t>(128, (B * n.out + 1023) / 1024);
  w.x = take(B * n.ld_x);
  w.h1 = take(B * n.hidden);
  w.pred = take(B * n.out);
  w.dpred = take(B * n.out);
  w.dh1 = take(B * n.hidden);
  w.dfeat = take(B * n.features);
  w.part = take((int64_t)w.grid * PPITCH);
  w.lossp = take(2 * 128);
  const int K1 = n.features + n.extra;
  const int64_t s1 = gemm_pick_splits(n.hidden, K1, batch, 1), s2 = gemm_pick_splits(n.out, n.hidden, batch, 1);
  w.gemm_floats = std::max(s1 * ((int64_t)n.hidden * K1 + n.hidden), s2 * ((int64_t)n.out * n.hidden + n.out));
  w.gemm = take(w.gemm_floats);
  w.total = o;
  return w;
}

const char* net_problem(const lrl_vision_net* n) {
  if (!n) return "lrl_vision: null net";
  const Map m = lds_map(n->height, n->width);
  if (n->height < 16 || n->height % 8 || n->width < 16 || n->width % 8 || n->height * n->width > 3072 ||
      n->hidden < 16 || n->hidden > 256 || n->hidden % 16 || n->out < 1 || n->out > 256 || n->extra < 0 ||
      n->extra > 256 || n->features != C3 * m.n3 || n->ld_x < n->features + n->extra || n->total <= 0)
    return "lrl_vision: the net was not filled by lrl_vision_net_init";
  return nullptr;
}

VisionK kernel_args(const lrl_vision_net& n, const float* params, const float* images, const float* extra,
                    int64_t ld_extra, const int64_t* rows, int batch, float* ws, const Ws& w) {
  VisionK k{};
  k.params = params; k.images = images; k.extra = extra; k.rows = rows;
  k.x = ws + w.x;
  k.c1w = n.c1w; k.c1b = n.c1b; k.c2w = n.c2w; k.c2b = n.c2b; k.c3w = n.c3w; k.c3b = n.c3b;
  k.ld_extra = ld_extra;
  k.H = n.height; k.W = n.width; k.E = n.extra; k.F = n.features; k.ldx = n.ld_x; k.batch = batch;
  k.scale = n.input_scale;
  return k;
}

bool lds_attr() {
  static const bool ok = [] {
    auto set = [](const void* f) {
      return hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
    };
    return set(reinterpret_cast<const void*>(vision_fwd_kernel)) && set(reinterpret_cast<const void*>(vision_bwd_kernel));
  }();
  return ok;
}

// one dense product through the descriptor path
int dense(int layout, int epi, int M, int N, int K, const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
          int64_t ldc, float* bias, const float* aux, int64_t ld_aux, float* gws, int64_t gws_floats, void* stream) {
  lrl_gemm_desc d{};
  d.layout = layout; d.epi = epi; d.M = M; d.N = N; d.K = K; d.groups = 1;
  d.A = A; d.B = B; d.C = C; d.bias = bias; d.aux = aux;
  d.lda = lda; d.ldb = ldb; d.ldc = ldc; d.ld_aux = ld_aux;
  d.workspace = gws; d.workspace_floats = gws_floats;
  return lrl_gemm_f32_ex(&d, stream);
}

// conv stack and the two dense layers: pred [batch][out] at `pred`
int forward(const lrl_vision_net& n, const float* params, const float* images, const float* extra, int64_t ld_extra,
            const int64_t* rows, int batch, float* pred, float* features, float* ws, const Ws& w, hipStream_t st) {
  if (!lds_attr()) return lrl_set_error(LRL_E_HIP, "lrl_vision: LDS attribute");
  VisionK k = kernel_args(n, params, images, extra, ld_extra, rows, batch, ws, w);
  k.features = features;
  const Map m = lds_map(n.height, n.width);
  hipLaunchKernelGGL(vision_fwd_kernel, dim3(w.grid), dim3(VT), (size_t)m.total * sizeof(float), st, k);
  if (hipGetLastError() != hipSuccess) return lrl_set_error(LRL_E_HIP, "lrl_vision: conv launch failed");
  float* P = const_cast<float*>(params);
  const int K1 = n.features + n.extra;
  if (int rc = dense(GEMM_NT, EPI_BIAS_ELU, batch, n.hidden, K1, ws + w.x, n.ld_x, params + n.f1w, K1, ws + w.h1,
                     n.hidden, P + n.f1b, nullptr, 0, nullptr, 0, st))
    return rc;
  return dense(GEMM_NT, EPI_BIAS, batch, n.out, n.hidden, ws + w.h1, n.hidden, params + n.f2w, n.hidden, pred, n.out,
               P + n.f2b, nullptr, 0, nullptr, 0, st);
}

const char* batch_problem(const lrl_vision_net* net, const void* params, const void* images, const void* extra,
                          int64_t ld_extra, int batch, const void* ws) {
  if (const char* e = net_problem(net)) return e;
  if (!params || !images || !ws || batch < 1) return "lrl_vision: null argument or batch < 1";
  if (net->extra > 0 && (!extra || ld_extra < net->extra)) return "lrl_vision: extra is null or ld_extra < extra";
  return nullptr;
}

}  // namespace

}  // namespace lrl

using namespace lrl;

extern "C" int32_t lrl_vision_net_init(lrl_vision_net* net, int32_t height, int32_t width, int32_t extra,
                                       int32_t hidden, int32_t out, float input_scale) {
  if (!net) return lrl_set_error(LRL_E_INVALID, "lrl_vision_net_init: null net");
  if (height < 16 || height % 8) return lrl_set_error(LRL_E_INVALID, "lrl_vision_net_init: height must be a multiple of 8, at least 16");
  if (width < 16 || width % 8) return lrl_set_error(LRL_E_INVALID, "lrl_vision_net_init: width must be a multiple of 8, at least 16");
  if (height * width > 3072) return lrl_set_error(LRL_E_INVALID, "lrl_vision_net_init: height * width must be at most 3072");
  if (extra < 0 || extra > 256) return lrl_set_error(LRL_E_INVALID, "lrl_vision_net_init: extra must be in [0, 256]");
  if (hidden < 16 || hidden > 256 || hidden % 16)
    return lrl_set_error(LRL_E_INVALID, "lrl_vision_net_init: hidden must be a multiple of 16 in [16, 256]");
  if (out < 1 || out > 256) return lrl_set_error(LRL_E_INVALID, "lrl_vision_net_init: out must be in [1, 256]");
  if (!(fabsf(input_scale) < 3e38f)) return lrl_set_error(LRL_E_INVALID, "lrl_vision_net_init: input_scale must be finite");
  lrl_vision_net n{};
  n.height = height; n.width = width; n.extra = extra; n.hidden = hidden; n.out = out; n.input_scale = input_scale;
  n.features = height * width / 2;
  n.ld_x = n.features + (extra + 3) / 4 * 4;
  int64_t off = 0;
  auto put = [&](int64_t count) { off = up64(off); const int64_t at = off; off += count; return at; };
  n.c1w = put(C1 * 25); n.c1b = put(C1);
  n.c2w = put(C2 * C1 * 9); n.c2b = put(C2);
  n.c3w = put(C3 * C2 * 9); n.c3b = put(C3);
  n.f1w = put((int64_t)hidden * (n.features + extra)); n.f1b = put(hidden);
  n.f2w = put((int64_t)out * hidden); n.f2b = put(out);
  n.total = up64(off);
  *net = n;
  return 0;
}

extern "C" int64_t lrl_vision_workspace_bytes(const lrl_vision_net* net, int32_t batch) {
  if (net_problem(net) || batch < 1) return 0;
  return ws_layout(*net, batch).total * (int64_t)sizeof(float);
}

extern "C" int32_t lrl_debug_vision_partials(const lrl_vision_net* net, int32_t batch, int64_t* offset_floats,
                                             int32_t* rows, int32_t* pitch, int32_t* used) {
  if (const char* e = net_problem(net)) return lrl_set_error(LRL_E_INVALID, e);
  if (batch < 1) return lrl_set_error(LRL_E_INVALID, "lrl_debug_vision_partials: batch < 1");
  const Ws w = ws_layout(*net, batch);
  if (offset_floats) *offset_floats = w.part;
  if (rows) *rows = w.grid;
  if (pitch) *pitch = PPITCH;
  if (used) *used = PCONV;
  return 0;
}

extern "C" int32_t lrl_vision_forward(const lrl_vision_net* net, const float* params, const float* images,
                                      const float* extra, int64_t ld_extra, const int64_t* rows, int32_t batch,
                                      float* out, float* features, void* workspace, void* stream) {
  if (const char* e = batch_problem(net, params, images, extra, ld_extra, batch, workspace))
    return lrl_set_error(LRL_E_INVALID, e);
  if (!out) return lrl_set_error(LRL_E_INVALID, "lrl_vision_forward: null out");
  const Ws w = ws_layout(*net, batch);
  return forward(*net, params, images, extra, ld_extra, rows, batch, out, features, static_cast<float*>(workspace), w,
                 static_cast<hipStream_t>(stream));
}

extern "C" int32_t lrl_vision_forward_backward(const lrl_vision_net* net, const float* params, float* grads,
                                               const float* images, const float* extra, int64_t ld_extra,
                                               const float* target, int64_t ld_target, const int64_t* rows,
                                               int32_t batch, double* loss_dev, void* workspace, void* stream) {
  if (const char* e = batch_problem(net, params, images, extra, ld_extra, batch, workspace))
    return lrl_set_error(LRL_E_INVALID, e);
  if (!grads || !target || !loss_dev || ld_target < net->out)
    return lrl_set_error(LRL_E_INVALID, "lrl_vision_forward_backward: null argument or ld_target < out");
  const lrl_vision_net& n = *net;
  const Ws w = ws_layout(n, batch);
  float* ws = static_cast<float*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = forward(n, params, images, extra, ld_extra, rows, batch, ws + w.pred, nullptr, ws, w, st)) return rc;
  const int64_t total = (int64_t)batch * n.out;
  double* lp = reinterpret_cast<double*>(ws + w.lossp);
  hipLaunchKernelGGL(vision_loss_kernel, dim3(w.loss_grid), dim3(256), 0, st, ws + w.pred, target, ld_target, rows, total,
                     n.out, 2.f / (float)total, ws + w.dpred, lp);
  hipLaunchKernelGGL(vision_loss_finish_kernel, dim3(1), dim3(64), 0, st, lp, w.loss_grid, 1.0 / (double)total, loss_dev);
  if (hipGetLastError() != hipSuccess) return lrl_set_error(LRL_E_HIP, "lrl_vision_forward_backward: loss launch failed");
  const int K1 = n.features + n.extra;
  float* gw = ws + w.gemm;
  // fc2: dW2 = d_pred^T h, db2; dh = (d_pred W2) * elu'(h)
  if (int rc = dense(GEMM_TN, EPI_PARTIAL, n.out, n.hidden, batch, ws + w.dpred, n.out, ws + w.h1, n.hidden,
                     grads + n.f2w, n.hidden, grads + n.f2b, nullptr, 0, gw, w.gemm_floats, st))
    return rc;
  if (int rc = dense(GEMM_NN, EPI_DELU, batch, n.hidden, n.out, ws + w.dpred, n.out, params + n.f2w, n.hidden,
                     ws + w.dh1, n.hidden, nullptr, ws + w.h1, n.hidden, nullptr, 0, st))
    return rc;
  // fc1: dW1 = dh^T [features | extra], db1; d_features = dh W1[:, :F]
  if (int rc = dense(GEMM_TN, EPI_PARTIAL, n.hidden, K1, batch, ws + w.dh1, n.hidden, ws + w.x, n.ld_x, grads + n.f1w, K1,
                     grads + n.f1b, nullptr, 0, gw, w.gemm_floats, st))
    return rc;
  if (int rc = dense(GEMM_NN, EPI_STORE, batch, n.features, n.hidden, ws + w.dh1, n.hidden, params + n.f1w, K1,
                     ws + w.dfeat, n.features, nullptr, nullptr, 0, nullptr, 0, st))
    return rc;
  VisionK k = kernel_args(n, params, images, extra, ld_extra, rows, batch, ws, w);
  k.dfeat = ws + w.dfeat;
  k.partials = ws + w.part;
  const Map m = lds_map(n.height, n.width);
  hipLaunchKernelGGL(vision_bwd_kernel, dim3(w.grid), dim3(VT), (size_t)m.total * sizeof(float), st, k);
  hipLaunchKernelGGL(vision_reduce_kernel, dim3((PCONV + 255) / 256), dim3(256), 0, st, ws + w.part, w.grid, grads, n.c1w,
                     n.c1b, n.c2w, n.c2b, n.c3w, n.c3b);
  return hipGetLastError() == hipSuccess ? 0 : lrl_set_error(LRL_E_HIP, "lrl_vision_forward_backward: launch failed");
}
