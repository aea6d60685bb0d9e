/*
 * mli_lpips.h -- C ABI of the LPIPS (v0.1, AlexNet) op in libmli_hip.so.
 *
 * Same conventions as mli_metrics.h: int mli_<op>(const args*, mli_stream_t) returning a hipError_t
 * value, caller-owned buffers, no allocation and no synchronisation inside the library, a host-only
 * mli_<op>_workspace query, hipErrorInvalidValue without a launch for a NULL buffer, both or neither
 * of an input pair, or a shape outside the stated limits.  Versioned on its own
 * (MLI_LPIPS_ABI_VERSION): no other ABI changes with it.
 *
 * Replaces the lpips.LPIPS(net='alex') call of projects/NeuralLumen/scripts/compute_metrics.py.  The
 * library carries no weights: the caller hands the raw fp32 tensors of a weight file it holds to
 * mli_lpips_pack once and the packed buffer to every mli_lpips.  DESIGN.md §20 states every definition.
 *
 * Inputs are B pairs of 3-plane images [B][3][H*W], row-major, values in [0, 1]:
 *   fp32 v as it is;  uint8 v -> float(double(v) / 255.0).
 * Limits: MLI_LPIPS_MIN_SIDE <= H, W <= MLI_LPIPS_MAX_SIDE, 1 <= B <= MLI_LPIPS_MAX_PAIRS.  31 is the
 * smallest side that leaves the second pool a 3 x 3 input (spatial sizes 7 -> 3 -> 3 -> 1 -> 1).
 *
 * The network, on the 2B images (image i < B: prediction i, image B + i: target i):
 *   1. with normalize: v = 2*v - 1.  Scaling: (v - shift[c]) / scale[c].  fp32 IEEE operations in this
 *      order, no contraction.  The convolution pads with zero in the scaled space.
 *   2. layer   Cin -> Cout   kernel  stride  pad      a 3 x 3 stride-2 max-pool (no padding, floor)
 *        1       3 ->  64      11      4      2       stands before layers 2 and 3; every layer is
 *        2      64 -> 192       5      1      2       convolution + bias, then ReLU; the five taps are
 *        3     192 -> 384       3      1      1       the ReLU outputs.  A convolution output is the
 *        4     384 -> 256       3      1      1       fp32 fmaf chain over k = (kh, kw, ci) ascending,
 *        5     256 -> 256       3      1      1       starting from 0; the bias is added after it.
 *   3. per tap l and pixel, in double from the fp32 taps (x: prediction, y: target):
 *        nx = sqrt(sum_c x_c^2), ny likewise,
 *        d  = sum_c lin_l[c] * (x_c / (nx + 1e-10) - y_c / (ny + 1e-10))^2
 *      layers[b][l] = the mean of d over the tap's pixels; lpips[b] = layers[b][0] + ... + layers[b][4],
 *      added in that order.
 * No atomics: the same input gives the same bits, and a pair's bits do not depend on its batch.
 */
#ifndef MLI_LPIPS_H
#define MLI_LPIPS_H

#include <stdint.h>

#include "mli_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLI_LPIPS_ABI_VERSION 1
int mli_lpips_abi_version(void);

#define MLI_LPIPS_MIN_SIDE 31
#define MLI_LPIPS_MAX_SIDE 4096
#define MLI_LPIPS_MAX_PAIRS 64
#define MLI_LPIPS_LAYERS 5
#define MLI_LPIPS_TILE_M 64   /* output pixels per workgroup of the convolution */
#define MLI_LPIPS_TILE_N 64   /* output channels per workgroup; divides 64, 192, 384 and 256 */
#define MLI_LPIPS_TILE_K 16   /* K per LDS stage; divides every Cin but layer 1's, whose K = 363 is padded */
#define MLI_LPIPS_K1_PADDED 368
#define MLI_LPIPS_DIST_PIXELS 16 /* tap pixels per workgroup partial of the distance pass */

/* The raw weights, fp32 on the device: w[l] OIHW [Cout][Cin][k][k], b[l] [Cout], lin[l] [Cout],
 * shift [3], scale [3].  packed (mli_lpips_pack_workspace bytes) receives, per layer, the weights as
 * [K][Cout] with K ordered (kh, kw, ci) -- layer 1's rows 363 .. 367 zero -- then the biases, the
 * lin vectors, shift and scale. */
typedef struct {
  const float* w[MLI_LPIPS_LAYERS];
  const float* b[MLI_LPIPS_LAYERS];
  const float* lin[MLI_LPIPS_LAYERS];
  const float* shift;
  const float* scale;
  float* packed;
} mli_lpips_pack_args;
int mli_lpips_pack(const mli_lpips_pack_args* a, mli_stream_t s);
/* bytes[0]: packed. */
int mli_lpips_pack_workspace(const mli_lpips_pack_args* a, int64_t* bytes);

typedef struct {
  int B, H, W;
  int normalize; /* flag, 0 or 1 */
  /* exactly one of each pair */
  const float* pred_f32; /* [B][3][H*W] */
  const uint8_t* pred_u8;
  const float* target_f32; /* [B][3][H*W] */
  const uint8_t* target_u8;
  const float* packed; /* what mli_lpips_pack wrote */
  double* lpips;       /* [B] */
  double* layers;      /* [B][5] */
  /* all or none; channel-last [2B][h][w][C]: taps[0] the scaled input (C = 3, h x w = H x W),
   * taps[1 .. 5] the five taps */
  float* taps[MLI_LPIPS_LAYERS + 1];
  void* scratch; /* mli_lpips_workspace bytes, 16-byte aligned */
} mli_lpips_args;
int mli_lpips(const mli_lpips_args* a, mli_stream_t s);
/* bytes[0]: scratch. */
int mli_lpips_workspace(const mli_lpips_args* a, int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif
