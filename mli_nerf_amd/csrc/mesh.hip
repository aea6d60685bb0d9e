// Iso-surface extraction (marching cubes) -- include/mli_mesh.h.
//
// Four launches over one lattice block, slots from scans (no atomics, bit-reproducible):
//   mc_count_kernel  one thread per lattice point: its three forward-edge flags and, for a cell
//                    origin, the case's triangle count; 64-bit ballots per wave, LDS per
//                    workgroup, one (vertices, triangles) total per 256-point chunk
//   mc_scan_kernel   one workgroup: exclusive scan of the chunk totals in place + the grand totals
//   mc_emit_kernel   recomputes the flags, slot = chunk base + wave base + ballot rank; writes the
//                    vertex positions, the vertex keys and the edge -> slot map
//   mc_tris_kernel   recomputes the case; three slots per triangle from the map + the face keys
// Points are numbered with the lattice's smallest-stride axis fastest (McOrder), so a wave reads
// consecutive addresses; each point reads its 7 forward neighbours (the same lines its
// neighbours read: L1 / L2 hits), i.e. 4 B of new data per point and pass.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MLI_MC_QUAL static __device__ const
#include "mc_table.h"
#include "mli_mesh.h"

#define MLI_FI __device__ __forceinline__

namespace {

constexpr int CHUNK = MLI_MC_CHUNK;  // points per workgroup pass
constexpr int WAVES = CHUNK / 64;
constexpr int MAX_BLOCKS = 2048;     // memory-bound: cap the grid, stride the rest
constexpr int SCAN_THREADS = 1024;

// point numbering: id = q0 + n0 * (q1 + n1 * q2), q0 along axis a0 (the smallest stride)
struct McOrder {
  int a0, a1, a2;
  int n0, n1;
  int points, chunks;
};

struct McPoint {
  int i, j, k;       // block-local lattice index
  bool hx, hy, hz;   // the forward neighbour along each axis exists
  float v0, vx, vy, vz;
  uint32_t eflags;   // bit d: the edge to the +d neighbour changes sign
  uint32_t kase;     // 8-bit case (cell origins only)
  bool cell;
};

MLI_FI McPoint mc_point(const mli_mc_args& a, const McOrder& o, int id) {
  McPoint p;
  const bool valid = id < o.points;
  const int idc = valid ? id : 0;
  const int q0 = idc % o.n0, rest = idc / o.n0;
  const int q1 = rest % o.n1, q2 = rest / o.n1;
  p.i = o.a0 == 0 ? q0 : (o.a1 == 0 ? q1 : q2);
  p.j = o.a0 == 1 ? q0 : (o.a1 == 1 ? q1 : q2);
  p.k = o.a0 == 2 ? q0 : (o.a1 == 2 ? q1 : q2);
  p.hx = valid && p.i + 1 < a.nx;
  p.hy = valid && p.j + 1 < a.ny;
  p.hz = valid && p.k + 1 < a.nz;
  const float* s = a.sdf + ((int64_t)p.i * a.sx + (int64_t)p.j * a.sy + (int64_t)p.k * a.sz);
  const float iso = a.iso;
  // only `s < iso` classifies: NaN and s == iso are outside
  p.v0 = s[0];
  p.vx = p.hx ? s[a.sx] : p.v0;
  p.vy = p.hy ? s[a.sy] : p.v0;
  p.vz = p.hz ? s[a.sz] : p.v0;
  const bool in0 = p.v0 < iso;
  const bool inx = p.vx < iso, iny = p.vy < iso, inz = p.vz < iso;
  p.eflags = valid ? ((p.hx && in0 != inx) ? 1u : 0u) | ((p.hy && in0 != iny) ? 2u : 0u) |
                         ((p.hz && in0 != inz) ? 4u : 0u)
                   : 0u;
  p.cell = p.hx && p.hy && p.hz;
  p.kase = 0;
  if (p.cell) {
    const bool c3 = s[a.sx + a.sy] < iso, c5 = s[a.sx + a.sz] < iso, c6 = s[a.sy + a.sz] < iso;
    const bool c7 = s[a.sx + a.sy + a.sz] < iso;
    p.kase = (in0 ? 1u : 0u) | (inx ? 2u : 0u) | (iny ? 4u : 0u) | (c3 ? 8u : 0u) | (inz ? 16u : 0u) |
             (c5 ? 32u : 0u) | (c6 ? 64u : 0u) | (c7 ? 128u : 0u);
  }
  return p;
}

MLI_FI uint64_t lanes_below() {
  const int lane = threadIdx.x & 63;
  return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

// Per-wave totals and this lane's ranks.  Vertices are numbered axis-major within a wave (all x
// edges, then y, then z), triangles lane-major.
struct McRank {
  int wave_verts, wave_tris;
  int vrank[3];  // slot of this lane's edge d, relative to the wave
  int trank;     // first triangle slot of this lane, relative to the wave
};

MLI_FI McRank mc_rank(uint32_t eflags, uint32_t ntri) {
  const uint64_t below = lanes_below();
  const uint64_t bx = __ballot(eflags & 1u), by = __ballot(eflags & 2u), bz = __ballot(eflags & 4u);
  const uint64_t t0 = __ballot(ntri & 1u), t1 = __ballot(ntri & 2u), t2 = __ballot(ntri & 4u);
  McRank r;
  const int nx = __popcll(bx), ny = __popcll(by), nz = __popcll(bz);
  r.wave_verts = nx + ny + nz;
  r.wave_tris = __popcll(t0) + 2 * __popcll(t1) + 4 * __popcll(t2);
  r.vrank[0] = __popcll(bx & below);
  r.vrank[1] = nx + __popcll(by & below);
  r.vrank[2] = nx + ny + __popcll(bz & below);
  r.trank = __popcll(t0 & below) + 2 * __popcll(t1 & below) + 4 * __popcll(t2 & below);
  return r;
}

__global__ __launch_bounds__(CHUNK) void mc_count_kernel(mli_mc_args a, McOrder o) {
  __shared__ uint8_t tri_count[256];
  __shared__ int wsum[WAVES][2];
  tri_count[threadIdx.x] = MLI_MC_TRI_COUNT[threadIdx.x];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int chunk = blockIdx.x; chunk < o.chunks; chunk += gridDim.x) {  // (uniform per workgroup)
    const McPoint p = mc_point(a, o, chunk * CHUNK + threadIdx.x);
    const McRank r = mc_rank(p.eflags, p.cell ? tri_count[p.kase] : 0u);
    if (lane == 0) {
      wsum[wave][0] = r.wave_verts;
      wsum[wave][1] = r.wave_tris;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      int t = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) t += wsum[w][threadIdx.x];
      a.chunk_base[2 * chunk + threadIdx.x] = t;
    }
    __syncthreads();
  }
}

// One workgroup: exclusive scan of chunk_base[chunks][2] in place, totals to counts[2].
__global__ __launch_bounds__(SCAN_THREADS) void mc_scan_kernel(int32_t* chunk_base, int32_t* counts, int chunks) {
  __shared__ int part[2][SCAN_THREADS];
  const int t = threadIdx.x;
  const int per = (chunks + SCAN_THREADS - 1) / SCAN_THREADS;
  const int lo = min(t * per, chunks), hi = min(lo + per, chunks);
  int sv = 0, st = 0;
  for (int c = lo; c < hi; ++c) {
    sv += chunk_base[2 * c];
    st += chunk_base[2 * c + 1];
  }
  part[0][t] = sv;
  part[1][t] = st;
  __syncthreads();
  for (int d = 1; d < SCAN_THREADS; d <<= 1) {  // inclusive scan of the per-thread sums
    const int av = t >= d ? part[0][t - d] : 0, at = t >= d ? part[1][t - d] : 0;
    __syncthreads();
    part[0][t] += av;
    part[1][t] += at;
    __syncthreads();
  }
  int bv = part[0][t] - sv, bt = part[1][t] - st;
  for (int c = lo; c < hi; ++c) {
    const int nv = chunk_base[2 * c], nt = chunk_base[2 * c + 1];
    chunk_base[2 * c] = bv;
    chunk_base[2 * c + 1] = bt;
    bv += nv;
    bt += nt;
  }
  if (t == SCAN_THREADS - 1) {
    counts[0] = part[0][t];
    counts[1] = part[1][t];
  }
}

// this workgroup's wave bases within the chunk, from the waves' totals
MLI_FI void wave_bases(int (&wsum)[WAVES][2], const McRank& r, int& vbase, int& tbase) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    wsum[wave][0] = r.wave_verts;
    wsum[wave][1] = r.wave_tris;
  }
  __syncthreads();
  vbase = tbase = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w)
    if (w < wave) {
      vbase += wsum[w][0];
      tbase += wsum[w][1];
    }
  __syncthreads();
}

__global__ __launch_bounds__(CHUNK) void mc_emit_kernel(mli_mc_args a, McOrder o) {
  __shared__ uint8_t tri_count[256];
  __shared__ int wsum[WAVES][2];
  tri_count[threadIdx.x] = MLI_MC_TRI_COUNT[threadIdx.x];
  __syncthreads();
  for (int chunk = blockIdx.x; chunk < o.chunks; chunk += gridDim.x) {
    const McPoint p = mc_point(a, o, chunk * CHUNK + threadIdx.x);
    const McRank r = mc_rank(p.eflags, p.cell ? tri_count[p.kase] : 0u);
    int vbase, tbase;
    wave_bases(wsum, r, vbase, tbase);
    vbase += a.chunk_base[2 * chunk];
    if (!p.eflags) continue;
    const int gi = a.off_x + p.i, gj = a.off_y + p.j, gk = a.off_z + p.k;
    const int64_t gpoint = ((int64_t)gi * a.gy + gj) * a.gz + gk;
    const int lpoint = (p.i * a.ny + p.j) * a.nz + p.k;  // < 2^31 / 3 (host check)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      if (!(p.eflags >> d & 1u)) continue;
      const int slot = vbase + r.vrank[d];
      a.edge_slot[3 * lpoint + d] = slot;
      if (slot < 0 || slot >= a.max_vertices) continue;
      const float s1 = d == 0 ? p.vx : (d == 1 ? p.vy : p.vz);
      const float t = (a.iso - p.v0) / (s1 - p.v0);
      // origin + (index + t e_axis) * spacing: the index offset first, two more roundings
      const float fx = (float)gi + (d == 0 ? t : 0.0f);
      const float fy = (float)gj + (d == 1 ? t : 0.0f);
      const float fz = (float)gk + (d == 2 ? t : 0.0f);
      a.verts[3 * (int64_t)slot + 0] = a.origin[0] + fx * a.spacing;
      a.verts[3 * (int64_t)slot + 1] = a.origin[1] + fy * a.spacing;
      a.verts[3 * (int64_t)slot + 2] = a.origin[2] + fz * a.spacing;
      a.vert_keys[slot] = gpoint * 3 + d;
    }
  }
}

__global__ __launch_bounds__(CHUNK) void mc_tris_kernel(mli_mc_args a, McOrder o) {
  __shared__ uint32_t tri_edges[256][4];  // 16 edge bytes per case
  __shared__ int wsum[WAVES][2];
  {
    const uint8_t* row = MLI_MC_TRI_EDGES[threadIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w)
      tri_edges[threadIdx.x][w] = (uint32_t)row[4 * w] | (uint32_t)row[4 * w + 1] << 8 |
                                  (uint32_t)row[4 * w + 2] << 16 | (uint32_t)row[4 * w + 3] << 24;
  }
  __syncthreads();
  for (int chunk = blockIdx.x; chunk < o.chunks; chunk += gridDim.x) {
    const McPoint p = mc_point(a, o, chunk * CHUNK + threadIdx.x);
    const uint8_t* edges = reinterpret_cast<const uint8_t*>(tri_edges[p.kase]);
    int ntri = 0;
    if (p.cell)
      while (ntri < 5 && edges[3 * ntri] != 255) ++ntri;
    const McRank r = mc_rank(0u, (uint32_t)ntri);
    int vbase, tbase;
    wave_bases(wsum, r, vbase, tbase);
    tbase += a.chunk_base[2 * chunk + 1] + r.trank;
    if (!ntri) continue;
    const int lpoint = (p.i * a.ny + p.j) * a.nz + p.k;
    const int64_t gcell = ((int64_t)(a.off_x + p.i) * a.gy + (a.off_y + p.j)) * a.gz + (a.off_z + p.k);
    for (int t = 0; t < ntri; ++t) {
      const int slot = tbase + t;
      if (slot < 0 || slot >= a.max_triangles) break;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int e = edges[3 * t + c];  // < 12 (table)
        const int q = lpoint + (MLI_MC_EDGE_CORNER[e][0] * a.ny + MLI_MC_EDGE_CORNER[e][1]) * a.nz +
                      MLI_MC_EDGE_CORNER[e][2];
        a.faces[3 * (int64_t)slot + c] = a.edge_slot[3 * q + MLI_MC_EDGE_AXIS[e]];
      }
      a.face_keys[slot] = gcell * 8 + t;
    }
  }
}

// shape limits of the ABI; fills the point order (smallest stride fastest)
bool mc_order(const mli_mc_args* a, McOrder* o) {
  if (a->nx < 2 || a->ny < 2 || a->nz < 2) return false;
  const int64_t points = (int64_t)a->nx * a->ny * a->nz;
  if (3 * points >= ((int64_t)1 << 31)) return false;
  if (a->sx < 0 || a->sy < 0 || a->sz < 0) return false;
  const int n[3] = {a->nx, a->ny, a->nz};
  const int64_t st[3] = {a->sx, a->sy, a->sz};
  int ax[3] = {0, 1, 2};
  for (int u = 0; u < 3; ++u)  // ascending stride; ties keep z fastest (a contiguous tensor's order)
    for (int v = u + 1; v < 3; ++v)
      if (st[ax[v]] < st[ax[u]] || (st[ax[v]] == st[ax[u]] && ax[v] > ax[u])) {
        const int tmp = ax[u];
        ax[u] = ax[v];
        ax[v] = tmp;
      }
  o->a0 = ax[0];
  o->a1 = ax[1];
  o->a2 = ax[2];
  o->n0 = n[ax[0]];
  o->n1 = n[ax[1]];
  o->points = (int)points;
  o->chunks = (int)((points + CHUNK - 1) / CHUNK);
  return true;
}

int mc_blocks(const McOrder& o) { return o.chunks < MAX_BLOCKS ? o.chunks : MAX_BLOCKS; }

}  // namespace

extern "C" int mli_mesh_abi_version(void) { return MLI_MESH_ABI_VERSION; }

extern "C" int mli_mc_count_workspace(const mli_mc_args* a, int64_t* bytes) {
  McOrder o;
  if (!mc_order(a, &o)) return (int)hipErrorInvalidValue;
  bytes[0] = (int64_t)o.chunks * 2 * sizeof(int32_t);
  bytes[1] = 2 * sizeof(int32_t);
  return 0;
}

extern "C" int mli_mc_emit_workspace(const mli_mc_args* a, int64_t* bytes) {
  McOrder o;
  if (!mc_order(a, &o)) return (int)hipErrorInvalidValue;
  bytes[0] = (int64_t)o.points * 3 * sizeof(int32_t);
  return 0;
}

extern "C" int mli_mc_count(const mli_mc_args* a, mli_stream_t s) {
  McOrder o;
  if (!mc_order(a, &o)) return (int)hipErrorInvalidValue;
  if (a->sdf == nullptr || a->chunk_base == nullptr || a->counts == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(mc_count_kernel, dim3(mc_blocks(o)), dim3(CHUNK), 0, (hipStream_t)s, *a, o);
  hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, (hipStream_t)s, a->chunk_base, a->counts,
                     o.chunks);
  return (int)hipGetLastError();
}

extern "C" int mli_mc_emit(const mli_mc_args* a, mli_stream_t s) {
  McOrder o;
  if (!mc_order(a, &o)) return (int)hipErrorInvalidValue;
  if (a->sdf == nullptr || a->chunk_base == nullptr || a->edge_slot == nullptr) return (int)hipErrorInvalidValue;
  if (a->max_vertices < 0 || a->max_triangles < 0) return (int)hipErrorInvalidValue;
  if (a->max_vertices > 0 && (a->verts == nullptr || a->vert_keys == nullptr)) return (int)hipErrorInvalidValue;
  if (a->max_triangles > 0 && (a->faces == nullptr || a->face_keys == nullptr)) return (int)hipErrorInvalidValue;
  if (a->max_vertices == 0 && a->max_triangles == 0) return 0;
  hipLaunchKernelGGL(mc_emit_kernel, dim3(mc_blocks(o)), dim3(CHUNK), 0, (hipStream_t)s, *a, o);
  hipLaunchKernelGGL(mc_tris_kernel, dim3(mc_blocks(o)), dim3(CHUNK), 0, (hipStream_t)s, *a, o);
  return (int)hipGetLastError();
}
