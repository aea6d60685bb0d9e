/*
 * mli_labels.h -- C ABI of the stage-b pseudo-label ops in libmli_hip.so.
 *
 * Same conventions as mli_hip.h / mli_mesh.h: int mli_<op>(const args*, mli_stream_t) returning a
 * hipError_t value, caller-owned buffers, no allocation and no synchronisation inside the library,
 * host-only mli_<op>_workspace queries for the scratch sizes, hipErrorInvalidValue without a launch
 * for a NULL buffer or a shape outside the stated limits.  Versioned on its own
 * (MLI_LABELS_ABI_VERSION): the rendering ABI and the mesh ABI do not change with it.
 *
 * Replaces projects/NeuralLumen/scripts/pseudo_label.py: erosion (27-34), edge_weight (47-54),
 * find_best_ref (57-83), rgb2opp (86-93), kmeans_cluster (96-122), fill_holes_kd (210-282) and
 * the per-camera sequence of its driver (346-418).  DESIGN.md §15 states every definition and
 * where it departs from the reference (the k-means is this project's own, deterministic).
 *
 * All arithmetic is fp32 without contraction.  Images are planes of H*W pixels, row-major
 * (pixel p = y*W + x); `B` or `L` planes of one camera are batched as [B][H*W].
 * Shape limits: 1 <= H, W <= MLI_LABELS_MAX_SIDE; 1 <= B, L <= MLI_LABELS_MAX_PLANES;
 * 0 <= radius <= MLI_LABELS_MAX_RADIUS; 1 <= K <= MLI_LABELS_MAX_K and K <= L.
 */
#ifndef MLI_LABELS_H
#define MLI_LABELS_H

#include <stdint.h>

#include "mli_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLI_LABELS_ABI_VERSION 1
int mli_labels_abi_version(void);

#define MLI_LABELS_MAX_SIDE 16384
#define MLI_LABELS_MAX_PLANES 4096
#define MLI_LABELS_MAX_RADIUS 15 /* erosion kernels up to 31 x 31, edge steps up to 15 */
#define MLI_LABELS_MAX_K 4
#define MLI_LABELS_TILE_X 32     /* mli_label_morph: pixels per workgroup tile */
#define MLI_LABELS_TILE_Y 8
#define MLI_LABELS_DONOR_TILE 256 /* mli_label_fill: donors per LDS tile */
#define MLI_LABELS_MAX_SLICES 64  /* mli_label_fill: donor slices (gridDim.y) */

/* Morphology of binary maps + the pseudo shading.
 *   d(p)       = the smallest r >= 1 whose (2r+1)^2 window around p, indices clamped to the image
 *                (replicate padding), holds both values; "none" when there is no such r <= radius
 *   eroded(p)  = 1 iff v(p) = 1 and d(p) > erode_radius            (erosion, kernel 2*erode_radius + 1)
 *   c(p)       = d(p) <= edge_step ? edge_step - d(p) + 1 : 0      (edge_weight's sum of edge maps)
 *   certainty  = 1 - c / max_image(c), 1 where that max is 0
 * and, when normal_x_light is given,
 *   shading    = normal_x_light * eroded [* inter_mask],   shading_gamma = powf(shading, inv_gamma).
 * Two launches: the tile pass (eroded, c, one max per tile), then a per-pixel pass in which every
 * workgroup reduces its image's tile maxima (integers: any order gives the same value). */
typedef struct {
  int B, H, W;
  int erode_radius, edge_step;
  const float* visibility;     /* [B][H*W], values 0 or 1 */
  float* eroded;               /* [B][H*W] */
  float* certainty;            /* [B][H*W] (holds c between the two launches) */
  int32_t* tile_max;           /* scratch (mli_label_morph_workspace) */
  /* optional group: all NULL, or normal_x_light, shading and shading_gamma set */
  const float* normal_x_light; /* [B][H*W] */
  const float* inter_mask;     /* [B][H*W] or NULL */
  float inv_gamma;
  float* shading;              /* [B][H*W] */
  float* shading_gamma;        /* [B][H*W] */
} mli_label_morph_args;
int mli_label_morph(const mli_label_morph_args* a, mli_stream_t s);
/* bytes[0]: tile_max. */
int mli_label_morph_workspace(const mli_label_morph_args* a, int64_t* bytes);

/* K-means along pixels: one problem per pixel, its L points x_l = (o1, o2),
 *   o1 = (r - g) / fp32(sqrt 2),  o2 = ((r + g) - 2*b) / fp32(sqrt 6),  d2 = dx*dx + dy*dy.
 * Centres start at c_0 = x_0, c_j = the point with the largest min_{i<j} d2(x_l, c_i) (lowest l on
 * ties).  A pass assigns every point to its nearest centre (lowest cluster on ties); when a pass
 * after the first changes no label the problem stops, otherwise every non-empty cluster's centre
 * becomes the sum of its members in ascending l divided by fp32(count), and after max_iter passes
 * it stops as well.  One thread per pixel, the points re-read from `image` every pass. */
typedef struct {
  int L, K, n_pixels, max_iter; /* max_iter >= 1 */
  const float* image;           /* [L][3][n_pixels] r, g, b planes */
  uint8_t* labels;              /* [L][n_pixels] */
  float* centers;               /* [K][2][n_pixels] */
  int32_t* passes;              /* [n_pixels] assignment passes run, or NULL */
} mli_label_kmeans_args;
int mli_label_kmeans(const mli_label_kmeans_args* a, mli_stream_t s);

/* find_best_ref per pixel.  mask_l = shading_l > threshold; a masked light's label counts as K.
 * Winners = the clusters with the most unmasked lights; g_l = light l is unmasked and in a winner;
 * smax = max_l(shading_l * g_l); keep_l = g_l and shading_l > fp32(threshold_wrt_max) * smax;
 * average_ref_c = sum_{keep, ascending l}(image_{l,c} / shading_gamma_l) / max(#keep, 1).  The
 * quotient is evaluated for kept lights only. */
typedef struct {
  int L, K, n_pixels;
  float threshold, threshold_wrt_max;
  const float* image;         /* [L][3][n_pixels] */
  const float* shading;       /* [L][n_pixels] */
  const float* shading_gamma; /* [L][n_pixels] */
  const uint8_t* labels;      /* [L][n_pixels], values < K */
  float* average_ref;         /* [3][n_pixels] */
  int32_t* keep_count;        /* [n_pixels] #keep */
  uint8_t* any_mask;          /* [n_pixels] any_l mask_l */
} mli_label_best_ref_args;
int mli_label_best_ref(const mli_label_best_ref_args* a, mli_stream_t s);

/* Nearest-donor fill.  Per pixel: 5 base features pos = (y, x) / fp32(max(H-1, W-1, 1)) * 4 and
 * n / (|n| + 1e-10), and the K colour features `centers`.  For hole h and donor p
 *   D(h, p) = |base_h - base_p|^2 + min_{i,j<K} |c_i(h) - c_j(p)|^2       (direct differences)
 * and ref[:, hole] = ref[:, argmin_p D], the lowest position in donor_idx on ties.  hole_idx and
 * donor_idx are disjoint lists of pixel indices.  Four launches: the two feature gathers, the
 * search (one thread per hole, donor tiles of MLI_LABELS_DONOR_TILE in LDS, the donors split into
 * `slices` ranges over gridDim.y, one packed (bits(D) << 32 | position) partial per hole and
 * slice), and the reduction of the partials in slice order with the copy.  The same input gives
 * the same bits.  n_holes = 0 launches nothing. */
typedef struct {
  int H, W, K;
  int n_holes, n_donors;   /* n_holes >= 0, n_donors >= 1 */
  int slices;              /* 0: chosen by the library; else 1 .. MLI_LABELS_MAX_SLICES */
  const float* normal;     /* [3][H*W] */
  const float* centers;    /* [K][2][H*W] */
  const int32_t* hole_idx; /* [n_holes] */
  const int32_t* donor_idx; /* [n_donors] */
  float* ref;              /* [3][H*W], filled in place */
  /* scratch (mli_label_fill_workspace) */
  float* hole_feat;
  float* donor_feat;
  uint64_t* partial;
} mli_label_fill_args;
int mli_label_fill(const mli_label_fill_args* a, mli_stream_t s);
/* bytes[0]: hole_feat, bytes[1]: donor_feat, bytes[2]: partial. */
int mli_label_fill_workspace(const mli_label_fill_args* a, int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif
