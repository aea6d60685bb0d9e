/*
 * mli_metrics.h -- C ABI of the image-metric op in libmli_hip.so.
 *
 * Same conventions as mli_hip.h / mli_mesh.h / mli_labels.h: int mli_<op>(const args*, mli_stream_t)
 * returning a hipError_t value, caller-owned buffers, no allocation and no synchronisation inside
 * the library, a host-only mli_<op>_workspace query for the scratch sizes, hipErrorInvalidValue
 * without a launch for a NULL buffer or a shape outside the stated limits.  Versioned on its own
 * (MLI_METRICS_ABI_VERSION): the rendering, mesh, mesh-CC and labels ABIs do not change with it.
 *
 * Replaces projects/NeuralLumen/scripts/compute_metrics.py:38-86 (calculate_metrics) without LPIPS:
 * the preparation of the two images (:40-57), skimage's peak_signal_noise_ratio and
 * mean_squared_error, and skimage's structural_similarity(channel_axis=-1, data_range=1.0).
 * DESIGN.md §17 states every definition.
 *
 * All arithmetic is IEEE double without contraction.  Images are B pairs of C planes of H*W pixels,
 * row-major (pixel p = y*W + x), laid out [B][C][H*W]; an alpha plane is [B][H*W].
 * Shape limits: 1 <= B <= MLI_METRICS_MAX_IMAGES; 1 <= C <= MLI_METRICS_MAX_CHANNELS;
 * MLI_METRICS_WINDOW <= H, W <= MLI_METRICS_MAX_SIDE.
 */
#ifndef MLI_METRICS_H
#define MLI_METRICS_H

#include <stdint.h>

#include "mli_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLI_METRICS_ABI_VERSION 1
int mli_metrics_abi_version(void);

#define MLI_METRICS_MAX_SIDE 16384
#define MLI_METRICS_MAX_IMAGES 16383 /* B * C planes ride on gridDim.z */
#define MLI_METRICS_MAX_CHANNELS 4
#define MLI_METRICS_WINDOW 7 /* the SSIM window; the tile's halo is WINDOW / 2 pixels */
#define MLI_METRICS_TILE_X 32 /* pixels per workgroup tile */
#define MLI_METRICS_TILE_Y 8

/* Preparation, per pixel (p: prediction, t: target, a: alpha of the pixel's image):
 *   uint8 v                -> double(v) / 255.0
 *   fp32 v, quantize       -> double(uint8(clamp(v, 0, 1) * 255.0f)) / 255.0   (fp32 product, truncated:
 *                             the 8-bit file relight.save_image writes)
 *   fp32 v, no quantize    -> double(v)
 *   alpha                  -> uint8 / 255.0, or double(fp32) (never quantised)
 *   with alpha             t = t * a + 1.0 * (1 - a); with mask_pred also p = p * a + 1.0 * (1 - a)
 *   with gamma_target      t = pow(t, inv_gamma)                (after the compositing)
 * Metrics, per image, on the prepared planes:
 *   mse  = sum_{c, pixel} (p - t)^2 / (C*H*W),   psnr = 10 * log10(1 / mse), +inf when mse = 0
 *   ssim_channels[c] = the mean over the (H-6) x (W-6) window centres 3 <= y < H-3, 3 <= x < W-3 of
 *     S = ((2*ux*uy + C1) * (2*vxy + C2)) / ((ux*ux + uy*uy + C1) * (vx + vy + C2)),
 *     ux, uy, uxx, uyy, uxy = the 7 x 7 window sums of p, t, p*p, t*t, p*t divided by 49 (each sum: the
 *     7 row sums left to right, then those top to bottom), vx = 49/48 * (uxx - ux*ux), vy and vxy
 *     likewise, C1 = 0.01^2, C2 = 0.03^2
 *   ssim = sum_c ssim_channels[c] / C
 * Two launches: the tile pass (one workgroup per MLI_METRICS_TILE_X x MLI_METRICS_TILE_Y pixel tile of
 * one (image, channel): the prepared tile and its 3-pixel halo as doubles in LDS, the five window sums
 * separably, one (sum of S, sum of squared error) partial per tile, reduced in a fixed order), then one
 * workgroup per image adding its partials in a fixed order.  No atomics: the same input gives the same
 * bits, and an image's results do not depend on the batch it is scored in. */
typedef struct {
  int B, C, H, W;
  int quantize, mask_pred, gamma_target; /* flags, 0 or 1; mask_pred needs an alpha plane */
  double inv_gamma;                      /* > 0 when gamma_target */
  /* exactly one of each pair */
  const float* pred_f32; /* [B][C][H*W] */
  const uint8_t* pred_u8;
  const float* target_f32; /* [B][C][H*W] */
  const uint8_t* target_u8;
  /* at most one of the pair */
  const float* alpha_f32; /* [B][H*W] */
  const uint8_t* alpha_u8;
  double* mse;           /* [B] */
  double* psnr;          /* [B] */
  double* ssim;          /* [B] */
  double* ssim_channels; /* [B][C] */
  double* prep_pred;     /* [B][C][H*W] the prepared prediction, or NULL */
  double* prep_target;   /* [B][C][H*W] the prepared target, or NULL */
  double* partial;       /* scratch (mli_image_metrics_workspace) */
} mli_image_metrics_args;
int mli_image_metrics(const mli_image_metrics_args* a, mli_stream_t s);
/* bytes[0]: partial. */
int mli_image_metrics_workspace(const mli_image_metrics_args* a, int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif
