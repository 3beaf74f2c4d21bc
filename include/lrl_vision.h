/* lrl_vision.h - the depth encoder's part of liblrl's C ABI (include/lrl.h includes this file; LRL_ABI_VERSION, the
 * LRL_E_* codes and lrl_last_error are declared there).  Appended entry points: no struct or function that existed
 * before changes, so LRL_ABI_VERSION stays. */
#ifndef LRL_VISION_H_
#define LRL_VISION_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Depth encoder (project-only; csrc/lrl_vision.hip, lrl/vision.py): a fixed convolution stack over one depth image
 * per sample and two dense layers, forward and MSE gradient.  Appended entry points: no struct or function that
 * existed before changes, so LRL_ABI_VERSION stays.
 *   x = depth * input_scale; torch cross-correlation on NCHW, ELU (alpha 1) after every layer but the last:
 *   conv1 1 -> 16, 5 x 5, stride 2, pad 2; conv2 16 -> 32, 3 x 3, stride 2, pad 1; conv3 32 -> 32, 3 x 3, stride 2,
 *   pad 1; flatten in (c, y, x) order (F = H W / 2 features); concatenate `extra` (E columns); fc1 F + E -> hidden;
 *   fc2 hidden -> out.
 *   envelope: H and W multiples of 8, each >= 16, H W <= 3072; hidden a multiple of 16 in [16, 256]; out in [1, 256];
 *   E in [0, 256].
 *   The three convolutions are one launch per direction: a workgroup keeps one image and its activation maps in LDS
 *   (30 H W bytes and one pad word per channel plane) and loops over the images beyond the grid; fp32 FMAs in a fixed
 *   order, so a feature row depends on its own image and the weights only.  The backward launch recomputes the maps,
 *   accumulates each workgroup's weight gradients in registers and writes one partial row per workgroup; a second
 *   launch adds the rows in workgroup order (no atomics: the same bits every call).  The dense layers are
 *   lrl_gemm_f32_ex products.
 *   parameters / grads: one flat fp32 buffer each, the fields in state_dict order (conv1.weight, conv1.bias, ...,
 *   fc2.weight, fc2.bias) at the offsets of the descriptor, every field aligned to 64 floats; a call writes every
 *   field of grads (it does not accumulate) and leaves the padding between fields alone.
 *   rows: NULL, or int64 dataset indices: sample i reads image, extra row and target row rows[i].
 * ------------------------------------------------------------------------------------------ */
#define LRL_VISION_MAX_WORKGROUPS 512 /* grid cap of the two conv-stack launches */
typedef struct lrl_vision_net {
  int32_t height, width, extra, hidden, out;
  float input_scale;
  int32_t features;                             /* F = height * width / 2 */
  int32_t ld_x;                                 /* pitch of a [features | extra] row in the workspace */
  int64_t c1w, c1b, c2w, c2b, c3w, c3b;         /* conv1..3 weight / bias, offsets in floats */
  int64_t f1w, f1b, f2w, f2b;                   /* fc1 [hidden][F + E], fc2 [out][hidden] */
  int64_t total;                                /* buffer length */
} lrl_vision_net;                               /* 120 bytes */
/* Host only: checks the envelope (LRL_E_INVALID and a message that names the violated bound) and fills the net. */
int32_t lrl_vision_net_init(lrl_vision_net* net, int32_t height, int32_t width, int32_t extra, int32_t hidden,
                            int32_t out, float input_scale);
/* Bytes of the workspace either call needs for `batch` samples (0 for a net lrl_vision_net_init did not fill). */
int64_t lrl_vision_workspace_bytes(const lrl_vision_net* net, int32_t batch);
/* out [batch][out] = the network's output; features (or NULL) [batch][F] receives the conv stack's output.
 * images [.][H][W], extra [.][ld_extra] (NULL when E = 0). */
int32_t lrl_vision_forward(const lrl_vision_net* net, const float* params, const float* images, const float* extra,
                           int64_t ld_extra, const int64_t* rows, int32_t batch, float* out, float* features,
                           void* workspace, void* stream);
/* grads = d loss / d params for loss = mean((pred - target)^2) over batch * out elements (F.mse_loss), *loss_dev (a
 * device double) = the loss, summed in a fixed order.  target [.][ld_target]. */
int32_t lrl_vision_forward_backward(const lrl_vision_net* net, const float* params, float* grads, const float* images,
                                    const float* extra, int64_t ld_extra, const float* target, int64_t ld_target,
                                    const int64_t* rows, int32_t batch, double* loss_dev, void* workspace,
                                    void* stream);
/* Where lrl_vision_forward_backward keeps the conv gradients' partial rows in its workspace: `rows` rows of `pitch`
 * floats from float `offset_floats`, the first `used` of each written (tests check the rest stays as it was). */
int32_t lrl_debug_vision_partials(const lrl_vision_net* net, int32_t batch, int64_t* offset_floats, int32_t* rows,
                                  int32_t* pitch, int32_t* used);

#ifdef __cplusplus
}
#endif
#endif /* LRL_VISION_H_ */
