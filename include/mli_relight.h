/*
 * mli_relight.h -- C ABI of the multi-light ops in libmli_hip.so: one camera view under L lights
 * with everything that does not depend on the light computed once.
 *
 * Same conventions as mli_hip.h / mli_mesh.h / mli_labels.h / mli_metrics.h:
 * int mli_<op>(const args*, mli_stream_t) returning a hipError_t value, caller-owned buffers, no
 * allocation and no synchronisation inside the library, hipErrorInvalidValue without a launch for a
 * NULL required buffer or a value outside the stated limits.  None of the three ops needs scratch, so
 * there is no workspace query.  Versioned on its own (MLI_RELIGHT_ABI_VERSION): the rendering, mesh,
 * mesh-CC, labels and metrics ABIs do not change with it.
 *
 * L <= 0 or R <= 0 returns 0 without a launch; L * R must not exceed INT32_MAX.
 * Every output holds, per light, the bits the per-light path (mli_rays + mli_light_visibility with
 * that light's pose) writes: the kernels share their arithmetic with it function by function.
 */
#ifndef MLI_RELIGHT_H
#define MLI_RELIGHT_H

#include <stdint.h>

#include "mli_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLI_RELIGHT_ABI_VERSION 1
int mli_relight_abi_version(void);

/* ---------------------------------------------------------------- light positions
 * Replaces the per-light half of NeuralLumen/utils/utils.py:61-79 (get_center_and_ray_lumen): the
 * light position, -R_l^T t_l of the w2l pose [R_l | t_l], repeated for every ray.  Row l of
 * pts_light holds what mli_rays writes to its pts_light when given pose_lights[l]. */
typedef struct {
  int L, R;
  const float* pose_lights; /* [L][3][4] world-to-light */
  float* pts_light;         /* [L][R][3] */
} mli_light_points_args;
int mli_light_points(const mli_light_points_args* a, mli_stream_t s);

/* ---------------------------------------------------------------- camera intersection
 * The camera half of mli_light_visibility (NeuralLumen/model.py:133-148): the intersection of every
 * camera ray with the surface, by camera_ray_type 0: sphere tracing from the composited depth,
 * 1: the composited depth itself, 2: sphere tracing from near (neuralangelo/model.py:298-325).
 * One launch.  blend_dist is read by types 0 and 1 only, the table / wsdf by types 0 and 2 only. */
typedef struct {
  int R;
  const float* center; const float* ray_unit;   /* [R,3] */
  const float* near_; const float* far_;        /* camera ray bounds [R] */
  const float* blend_dist;                      /* [R] from mli_composite_fwd */
  int camera_ray_type, iters;
  const uint16_t* table; mli_grid_levels levels; int active_levels; const void* wsdf;
  float* inter_dist; uint8_t* inter_mask; float* inter_pts;   /* [R],[R],[R,3] */
} mli_camera_hit_args;
int mli_camera_hit(const mli_camera_hit_args* a, mli_stream_t s);

/* ---------------------------------------------------------------- light rays, all lights
 * The light half of mli_light_visibility (NeuralLumen/model.py:149-184, :330-334) for all L * R
 * (light, ray) pairs p = l * R + r in one launch: the light ray from pts_light[l][r] to
 * inter_pts[r] over the visibility bounds (get_dist_bounds_visibility, model.py:186-199), `iters`
 * sphere-tracing steps along it, then visibility = !hit | !inside, normal_x_light =
 * relu(normalize(-gradient[r]) . light_dir), pseudo_shading = normal_x_light * visibility
 * (^ 1/gamma).  One wave handles 32 consecutive pairs; the light ray lives in registers. */
typedef struct {
  int L, R;
  const float* pts_light;  /* [L][R][3] (mli_light_points) */
  const float* inter_pts;  /* [R,3] (mli_camera_hit) */
  const float* gradient;   /* [R,3] composited gradients (eval) */
  int vis_box;             /* 0: sphere of radius^2 vis_r2, 1: the AABB */
  float vis_r2; float aabb[6];
  float gamma;             /* 0: none */
  int iters;
  const uint16_t* table; mli_grid_levels levels; int active_levels; const void* wsdf;
  uint8_t* visibility; float* normal_x_light; float* pseudo_shading;   /* [L][R] */
} mli_light_shadows_args;
int mli_light_shadows(const mli_light_shadows_args* a, mli_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
