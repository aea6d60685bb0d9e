/*
 * mli_mesh.h -- C ABI of the iso-surface extraction (marching cubes) in libmli_hip.so.
 *
 * Same conventions as mli_hip.h: int mli_<op>(const args*, hipStream_t) returning a hipError_t
 * value, caller-owned buffers, no allocation and no synchronisation inside the library, host-only
 * mli_<op>_workspace queries for the scratch sizes.  Versioned on its own (MLI_MESH_ABI_VERSION):
 * the rendering ABI of mli_hip.h does not change with it.
 *
 * Replaces mcubes.marching_cubes as the reference calls it (projects/neuralangelo/utils/mesh.py:
 * 119-123), with vertices identified across blocks so that the caller can weld them.
 *
 * The lattice: nx x ny x nz fp32 values, element (i, j, k) at sdf[i*sx + j*sy + k*sz] (element
 * strides, so both a contiguous [nx][ny][nz] tensor and mli_sdf's [k][i*ny + j] output are read
 * in place).  It is the block at global lattice offset (off_x, off_y, off_z) of a global lattice
 * of gx x gy x gz points whose point (0, 0, 0) is at `origin` and whose spacing is `spacing`.
 *
 * Classification: a point is INSIDE when s < iso (NaN and s == iso are outside).  One vertex per
 * lattice edge whose end points differ, at
 *     t = (iso - s0) / (s1 - s0),   x_d = origin_d + (fp32(g_d) + (d == axis ? t : 0)) * spacing
 * (fp32, no fused multiply-add; g = global index of the edge's lower point, s0 its value).
 *   vertex key = ((g_i*gy + g_j)*gz + g_k)*3 + axis          (int64; axis 0, 1, 2 = +x, +y, +z)
 *   face key   = ((c_i*gy + c_j)*gz + c_k)*8 + t             (int64; c = global index of the cell's
 *                origin point, t = the triangle's position in the cell's row of mc_table.h)
 * Triangles are oriented with their normal toward increasing s (out of the inside).
 *
 * Output slots come from prefix sums in a fixed order, not from atomics: the same input gives the
 * same bits.  The order itself is unspecified (sort by key for a canonical mesh).
 *
 * Sequence:  mli_mc_count -> (host reads counts[2]) -> mli_mc_emit, same args, same stream.
 */
#ifndef MLI_MESH_H
#define MLI_MESH_H

#include <stdint.h>

#include "mli_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLI_MESH_ABI_VERSION 1
int mli_mesh_abi_version(void);

#define MLI_MC_CHUNK 256 /* lattice points per scan chunk (one workgroup pass) */

typedef struct {
  const float* sdf;       /* the lattice */
  int nx, ny, nz;         /* >= 2 each; 3 * nx*ny*nz < 2^31 */
  int64_t sx, sy, sz;     /* element strides (>= 0) */
  float iso;
  float origin[3];        /* position of global lattice point (0, 0, 0) */
  float spacing;
  int off_x, off_y, off_z; /* global index of this block's point (0, 0, 0) */
  int gx, gy, gz;         /* global lattice dimensions (points) */
  /* scratch (mli_mc_count_workspace) */
  int32_t* chunk_base;    /* [chunks][2]: per-chunk vertex / triangle totals, scanned in place */
  int32_t* counts;        /* [2] n_vertices, n_triangles (device; the host reads it back) */
  /* mli_mc_emit only */
  int32_t* edge_slot;     /* scratch [3 * nx*ny*nz]: vertex slot of edge (point (i*ny + j)*nz + k, axis) */
  int max_vertices, max_triangles; /* capacity of the outputs; slots beyond are not written */
  float* verts;           /* [max_vertices][3] */
  int64_t* vert_keys;     /* [max_vertices] */
  int32_t* faces;         /* [max_triangles][3] vertex slots */
  int64_t* face_keys;     /* [max_triangles] */
} mli_mc_args;

/* Counts (2 launches: classify + per-workgroup totals, then one workgroup scans the totals).
 * hipErrorInvalidValue, without a launch, for a shape outside the limits above or a NULL buffer. */
int mli_mc_count(const mli_mc_args* a, mli_stream_t s);
/* bytes[0]: chunk_base, bytes[1]: counts. */
int mli_mc_count_workspace(const mli_mc_args* a, int64_t* bytes);

/* Vertices, keys and the edge map (1 launch), then the triangles (1 launch).  Needs the
 * chunk_base mli_mc_count left for the same lattice. */
int mli_mc_emit(const mli_mc_args* a, mli_stream_t s);
/* bytes[0]: edge_slot. */
int mli_mc_emit_workspace(const mli_mc_args* a, int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif
