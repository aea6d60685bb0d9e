// Connected components of a triangle mesh -- include/mli_mesh_cc.h.
//
//   cc_init_kernel    label[v] = v, the flags and the statistics zeroed
//   cc_faces_kernel   one thread per face: 6 gathers (label and label-of-label of its three
//                     vertices), then for each vertex the smaller of the other two's
//                     label-of-label goes to label[label[u]] and label[u] by atomicMin -- issued only
//                     where the values just read say it lowers the word
//   cc_verts_kernel   one thread per vertex: label[x] = min(label[x], label[label[x]])
//   cc_stats_kernel   one thread per face: q in fp64, a segmented sum over the runs of equal labels
//                     in a wave (ballot + __shfl_up), the waves' last runs merged through LDS, the
//                     merged run carried by thread 0 across the chunks its workgroup walks
// Labels only decrease and only to indices of the same component, so the plain (possibly stale)
// reads are safe; nothing in a launch waits for another workgroup.  All sums are integers: the
// results do not depend on the order of the atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mli_mesh_cc.h"

#pragma clang fp contract(off)

#define MLI_FI __device__ __forceinline__

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_BLOCKS = 2048;  // memory-bound: cap the grid, stride the rest

typedef unsigned long long u64;

__global__ __launch_bounds__(THREADS) void cc_init_kernel(mli_cc_args a) {
  const int64_t n = a.n_verts;
  const int64_t total = n + 1 > a.max_rounds ? n + 1 : a.max_rounds;
  for (int64_t i = blockIdx.x * (int64_t)THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * THREADS) {
    if (i < n) {
      a.label[i] = (int32_t)i;
      a.comp_faces[i] = 0;
      a.comp_area[i] = 0;
    }
    if (i == n) a.max_q[0] = 0;
    if (i < a.max_rounds) a.changed[i] = 0;
  }
}

// label[idx] = min(label[idx], m) when `seen`, the value just read there, says that lowers it;
// true when the atomic did lower the word
MLI_FI bool cc_lower(int32_t* label, int32_t idx, int32_t seen, int32_t m) {
  if (m >= seen) return false;
  return atomicMin(&label[idx], m) > m;
}

MLI_FI bool cc_index(const mli_cc_args& a, int32_t i) { return (uint32_t)i < (uint32_t)a.n_verts; }

MLI_FI void cc_flag(const mli_cc_args& a, bool ch) {
  if (__ballot(ch) != 0ull && (threadIdx.x & 63) == 0) a.changed[a.round] = 1;
}

MLI_FI bool cc_face(const mli_cc_args& a, int64_t f, int64_t (&v)[3]) {
  const uint64_t V = (uint64_t)a.n_verts;
  const int64_t* p = a.faces + 3 * f;
  v[0] = p[0];
  v[1] = p[1];
  v[2] = p[2];
  return (uint64_t)v[0] < V && (uint64_t)v[1] < V && (uint64_t)v[2] < V;
}

__global__ __launch_bounds__(THREADS) void cc_faces_kernel(mli_cc_args a) {
  bool ch = false;
  for (int64_t f = blockIdx.x * (int64_t)THREADS + threadIdx.x; f < a.n_faces; f += (int64_t)gridDim.x * THREADS) {
    int64_t v[3];
    if (!cc_face(a, f, v)) continue;
    int32_t l[3], g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) l[c] = a.label[v[c]];
    // labels are vertex indices, in [0, V) after mli_cc_init; anything else is not followed
    if (!cc_index(a, l[0]) || !cc_index(a, l[1]) || !cc_index(a, l[2])) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = a.label[l[c]];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int32_t m = min(g[(c + 1) % 3], g[(c + 2) % 3]);  // both pairs that end in vertex c
      ch |= cc_lower(a.label, l[c], g[c], m);
      ch |= cc_lower(a.label, (int32_t)v[c], l[c], m);
    }
  }
  cc_flag(a, ch);
}

__global__ __launch_bounds__(THREADS) void cc_verts_kernel(mli_cc_args a) {
  bool ch = false;
  for (int64_t x = blockIdx.x * (int64_t)THREADS + threadIdx.x; x < a.n_verts; x += (int64_t)gridDim.x * THREADS) {
    const int32_t l = a.label[x];
    if (!cc_index(a, l)) continue;
    ch |= cc_lower(a.label, (int32_t)x, l, a.label[l]);
  }
  cc_flag(a, ch);
}

MLI_FI u64 cc_face_q(const float* verts, const int64_t (&v)[3], double inv_unit) {
  const float* pa = verts + 3 * v[0];
  const float* pb = verts + 3 * v[1];
  const float* pc = verts + 3 * v[2];
  const double ax = pa[0], ay = pa[1], az = pa[2];
  const double ux = (double)pb[0] - ax, uy = (double)pb[1] - ay, uz = (double)pb[2] - az;
  const double wx = (double)pc[0] - ax, wy = (double)pc[1] - ay, wz = (double)pc[2] - az;
  const double cx = uy * wz - uz * wy;
  const double cy = uz * wx - ux * wz;
  const double cz = ux * wy - uy * wx;
  const double n2 = (cx * cx + cy * cy) + cz * cz;
  return (u64)llrint(0.5 * sqrt(n2) * inv_unit);
}

MLI_FI void cc_add(const mli_cc_args& a, int32_t lab, u64 q, int32_t cnt) {
  if (lab < 0 || cnt == 0) return;
  if (q) atomicAdd(reinterpret_cast<u64*>(a.comp_area) + lab, q);
  atomicAdd(&a.comp_faces[lab], cnt);
}

__global__ __launch_bounds__(THREADS) void cc_stats_kernel(mli_cc_args a, int chunks) {
  __shared__ int32_t w_label[WAVES], w_cnt[WAVES];
  __shared__ u64 w_q[WAVES], w_max[WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t c_label = -1, c_cnt = 0;  // thread 0: the run carried across waves and chunks
  u64 c_q = 0, c_max = 0;
  for (int chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {  // (uniform per workgroup)
    const int64_t f = (int64_t)chunk * THREADS + threadIdx.x;
    int32_t lab = -1, cnt = 0;
    u64 q = 0;
    int64_t v[3];
    if (f < a.n_faces && cc_face(a, f, v)) {
      lab = a.label[v[0]];
      if (cc_index(a, lab)) {
        cnt = 1;
        if (a.verts != nullptr) q = cc_face_q(a.verts, v, a.inv_unit);
      } else {
        lab = -1;
      }
    }
    // runs of equal labels among the wave's consecutive lanes; inclusive sums within each run
    const int32_t prev = __shfl_up(lab, 1);
    const uint64_t heads = __ballot(lane == 0 || prev != lab);
    u64 sq = q, mq = q;
    int32_t sc = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 vq = __shfl_up(sq, d);
      const int32_t vc = __shfl_up(sc, d);
      const u64 vm = __shfl_xor(mq, d);
      // lane - d is in this lane's run: no run head in lanes (lane - d, lane]
      if (lane >= d && ((heads >> (lane - d + 1)) & ((1ull << d) - 1ull)) == 0ull) {
        sq += vq;
        sc += vc;
      }
      mq = vm > mq ? vm : mq;
    }
    const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
    if (lane == 63) {  // the wave's last run goes on to the workgroup's merge
      w_label[wave] = lab;
      w_q[wave] = sq;
      w_cnt[wave] = sc;
      w_max[wave] = mq;
    } else if (tail) {
      cc_add(a, lab, sq, sc);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 0; w < WAVES; ++w) {
        if (w_label[w] != c_label) {
          cc_add(a, c_label, c_q, c_cnt);
          c_label = w_label[w];
          c_q = 0;
          c_cnt = 0;
        }
        c_q += w_q[w];
        c_cnt += w_cnt[w];
        c_max = w_max[w] > c_max ? w_max[w] : c_max;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    cc_add(a, c_label, c_q, c_cnt);
    if (c_max) atomicMax(reinterpret_cast<u64*>(a.max_q), c_max);
  }
}

// shape limits of the ABI
bool cc_shape(const mli_cc_args* a) {
  if (a->n_verts < 1) return false;  // int32: V < 2^31
  if (a->n_faces < 0 || a->n_faces >= ((int64_t)1 << 31)) return false;
  return a->max_rounds >= 1 && a->max_rounds <= MLI_CC_MAX_ROUNDS;
}

int cc_blocks(int64_t n) {
  const int64_t b = (n + THREADS - 1) / THREADS;
  return (int)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

}  // namespace

extern "C" int mli_mesh_cc_abi_version(void) { return MLI_MESH_CC_ABI_VERSION; }

extern "C" int mli_cc_init_workspace(const mli_cc_args* a, int64_t* bytes) {
  if (!cc_shape(a)) return (int)hipErrorInvalidValue;
  bytes[0] = (int64_t)a->n_verts * sizeof(int32_t);
  bytes[1] = (int64_t)a->max_rounds * sizeof(int32_t);
  bytes[2] = (int64_t)a->n_verts * sizeof(int32_t);
  bytes[3] = ((int64_t)a->n_verts + 1) * sizeof(int64_t);
  return 0;
}

extern "C" int mli_cc_init(const mli_cc_args* a, mli_stream_t s) {
  if (!cc_shape(a)) return (int)hipErrorInvalidValue;
  if (a->label == nullptr || a->changed == nullptr || a->comp_faces == nullptr || a->comp_area == nullptr ||
      a->max_q == nullptr)
    return (int)hipErrorInvalidValue;
  const int64_t total = (int64_t)a->n_verts + 1 > a->max_rounds ? (int64_t)a->n_verts + 1 : a->max_rounds;
  hipLaunchKernelGGL(cc_init_kernel, dim3(cc_blocks(total)), dim3(THREADS), 0, (hipStream_t)s, *a);
  return (int)hipGetLastError();
}

extern "C" int mli_cc_round(const mli_cc_args* a, mli_stream_t s) {
  if (!cc_shape(a)) return (int)hipErrorInvalidValue;
  if (a->round < 0 || a->round >= a->max_rounds) return (int)hipErrorInvalidValue;
  if (a->label == nullptr || a->changed == nullptr || (a->n_faces > 0 && a->faces == nullptr))
    return (int)hipErrorInvalidValue;
  if (a->n_faces > 0)
    hipLaunchKernelGGL(cc_faces_kernel, dim3(cc_blocks(a->n_faces)), dim3(THREADS), 0, (hipStream_t)s, *a);
  hipLaunchKernelGGL(cc_verts_kernel, dim3(cc_blocks(a->n_verts)), dim3(THREADS), 0, (hipStream_t)s, *a);
  return (int)hipGetLastError();
}

extern "C" int mli_cc_stats(const mli_cc_args* a, mli_stream_t s) {
  if (!cc_shape(a)) return (int)hipErrorInvalidValue;
  if (a->label == nullptr || a->comp_faces == nullptr || a->comp_area == nullptr || a->max_q == nullptr ||
      (a->n_faces > 0 && a->faces == nullptr))
    return (int)hipErrorInvalidValue;
  if (a->verts != nullptr && !(a->inv_unit > 0.0 && a->inv_unit < __builtin_inf())) return (int)hipErrorInvalidValue;
  if (a->n_faces == 0) return 0;
  const int chunks = (int)((a->n_faces + THREADS - 1) / THREADS);
  hipLaunchKernelGGL(cc_stats_kernel, dim3(cc_blocks(a->n_faces)), dim3(THREADS), 0, (hipStream_t)s, *a, chunks);
  return (int)hipGetLastError();
}
