/*
 * mli_mesh_cc.h -- C ABI of the connected components of a triangle mesh in libmli_hip.so.
 *
 * Same conventions as mli_hip.h / mli_mesh.h / mli_labels.h: int mli_<op>(const args*, mli_stream_t)
 * returning a hipError_t value, caller-owned buffers, no allocation and no synchronisation inside
 * the library, a host-only workspace query for the scratch sizes, hipErrorInvalidValue without a
 * launch for a NULL buffer or a shape outside the stated limits.  Versioned on its own
 * (MLI_MESH_CC_ABI_VERSION): the rendering, mesh and labels ABIs do not change with it.
 *
 * Replaces trimesh's split + area as the reference uses them for --keep_lcc
 * (projects/neuralangelo/scripts/extract_mesh.py:38, projects/neuralangelo/utils/mesh.py:151-158
 * filter_largest_cc), on the welded mesh instead of per block.  DESIGN.md §14.6 states every
 * definition below in full.
 *
 * Graph: vertices 0 .. V-1; two vertices are adjacent when some face names both.  The label of a
 * vertex is the smallest vertex index of its component; a face belongs to the component of its
 * first vertex; a vertex no face names is a component with 0 faces.
 *
 * Labelling: min-label propagation with pointer jumping on label[V], label[v] = v at the start.
 * One round, for every face and each ordered pair (u, v) of its vertices, with g = label[label[v]]:
 *     label[label[u]] = min(.., g),  label[u] = min(.., g);
 * then for every vertex x: label[x] = min(label[x], label[label[x]]).  Every write is an atomicMin,
 * issued only when a plain read says it would lower the word; changed[round] is set when some
 * atomicMin returned a value above the one it wrote.  Words only decrease, and only to indices of
 * the same component, so a stale read costs at most a needless atomic; a round that lowered nothing
 * read the true state and is the fixpoint (every label = its component's minimum).  The host reads
 * changed[round] and stops there.  No workgroup waits for another.
 *
 * Area: q = llrint(0.5 * sqrt(|(b-a) x (c-a)|^2) * inv_unit) per face, fp64 without contraction
 * from the fp32 coordinates, n2 = (cx*cx + cy*cy) + cz*cz; inv_unit = 2^(44-e) with 2^e >= the
 * squared diagonal of the vertices' bounding box, so q <= 2^43.  comp_area[label] is the int64 sum
 * of q (order-independent), comp_faces[label] the count, max_q the largest q.
 *
 * A face with an index outside [0, V) is outside the ABI; the kernels skip it (no access).
 *
 * Sequence:  mli_cc_init -> { mli_cc_round(round = r) -> host reads changed[r] } until 0
 *            -> mli_cc_stats, same buffers, same stream.
 */
#ifndef MLI_MESH_CC_H
#define MLI_MESH_CC_H

#include <stdint.h>

#include "mli_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MLI_MESH_CC_ABI_VERSION 1
int mli_mesh_cc_abi_version(void);

#define MLI_CC_MAX_ROUNDS 4096 /* upper limit of max_rounds (the default is 2*ceil(log2 V) + 8) */

typedef struct {
  const int64_t* faces; /* [n_faces][3] vertex indices (may be NULL when n_faces = 0) */
  int64_t n_faces;      /* 0 <= F < 2^31 */
  const float* verts;   /* [n_verts][3]; mli_cc_stats only, NULL: q = 0 for every face */
  int32_t n_verts;      /* 1 <= V < 2^31 */
  int32_t* label;       /* [n_verts] */
  int32_t* changed;     /* [max_rounds] */
  int32_t max_rounds, round; /* 1 <= max_rounds <= MLI_CC_MAX_ROUNDS; 0 <= round < max_rounds */
  int32_t* comp_faces;  /* [n_verts] faces per label */
  int64_t* comp_area;   /* [n_verts] sum of q per label */
  int64_t* max_q;       /* [1] */
  double inv_unit;      /* 2^(44-e); finite and > 0 */
} mli_cc_args;

/* label[v] = v; changed, comp_faces, comp_area and max_q zeroed (1 launch).  Replaces the start of
 * trimesh's mesh.split (utils/mesh.py:152). */
int mli_cc_init(const mli_cc_args* a, mli_stream_t s);
/* bytes[0]: label, bytes[1]: changed, bytes[2]: comp_faces, bytes[3]: comp_area followed by max_q
 * (one allocation of n_verts + 1 int64 words). */
int mli_cc_init_workspace(const mli_cc_args* a, int64_t* bytes);

/* One round (2 launches: one thread per face, then one per vertex; n_faces = 0: the second only).
 * Replaces the connected-component search inside mesh.split(only_watertight=False)
 * (utils/mesh.py:152). */
int mli_cc_round(const mli_cc_args* a, mli_stream_t s);

/* comp_faces, comp_area and max_q from the converged labels (1 launch, one thread per face;
 * n_faces = 0 launches nothing).  Lanes of a wave whose consecutive faces share a label combine
 * first, then the waves of a workgroup, then the chunks a workgroup walks: one atomic pair per run.
 * Replaces `areas = np.array([c.area for c in components])` (utils/mesh.py:153). */
int mli_cc_stats(const mli_cc_args* a, mli_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
