// Stage-b pseudo labels -- include/mli_labels.h.
//
//   morph_tile_kernel    one 32 x 8 pixel tile per workgroup, the tile and its halo as bytes in
//                        LDS; the distance d(p) to the nearest pixel of the other value is found
//                        separably (per row the nearest 0 and the nearest 1, then the column scan),
//                        which gives the erosion and the edge count c at once + the tile's max c
//   morph_finish_kernel  per pixel: certainty = 1 - c / max_image(c) (every workgroup reduces its
//                        image's tile maxima: integers, order-free) and the pseudo shading
//   kmeans_kernel        one thread per pixel, the L points re-read (coalesced across pixels)
//                        every pass, the K centres, sums and counts in registers
//   best_ref_kernel      one thread per pixel, three passes over its L lights
//   fill_feat_kernel     feature rows (5 + 2K floats, padded to a multiple of 4) of listed pixels
//   fill_search_kernel   one thread per hole (features in registers), donor tiles in LDS read at
//                        wave-uniform addresses (broadcast, no bank conflicts), donors sliced
//                        over gridDim.y; one packed (D, position) partial per hole and slice
//   fill_reduce_kernel   the partials' minimum in slice order; copies the donor's reflectance
// No atomics on global memory and no floating-point reduction whose order depends on the launch:
// the same input gives the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mli_labels.h"

#define MLI_FI __device__ __forceinline__

namespace {

constexpr int TX = MLI_LABELS_TILE_X, TY = MLI_LABELS_TILE_Y;
constexpr int RMAX = MLI_LABELS_MAX_RADIUS;
constexpr int KMAX = MLI_LABELS_MAX_K;
constexpr int THREADS = 256;
constexpr int DTILE = MLI_LABELS_DONOR_TILE;
constexpr int HALO_ROWS = TY + 2 * RMAX;       // 38
constexpr int HALO_COLS = TX + 2 * RMAX + 2;   // 64 (62 used)
constexpr uint8_t NONE = 255;

// ------------------------------------------------------------------------------ morphology
__global__ __launch_bounds__(THREADS) void morph_tile_kernel(mli_label_morph_args a, int tiles_x, int tiles_y) {
  __shared__ uint8_t t[HALO_ROWS][HALO_COLS];   // 0 / 1, 2 outside the image
  __shared__ uint8_t hd[2][HALO_ROWS][TX];      // per row: distance to the nearest 0 / 1, NONE
  __shared__ int block_max;
  const int R = max(a.erode_radius, a.edge_step);
  const int tid = threadIdx.y * TX + threadIdx.x;
  const int b = blockIdx.z;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const size_t plane = (size_t)b * a.H * a.W;
  const int rows = TY + 2 * R, cols = TX + 2 * R;
  if (tid == 0) block_max = 0;
  for (int i = tid; i < rows * cols; i += THREADS) {
    const int ly = i / cols, lx = i - ly * cols;
    const int gy = y0 + ly - R, gx = x0 + lx - R;
    uint8_t v = 2;
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) v = a.visibility[plane + (size_t)gy * a.W + gx] != 0.0f ? 1 : 0;
    t[ly][lx] = v;
  }
  __syncthreads();
  for (int i = tid; i < rows * TX; i += THREADS) {
    const int row = i / TX, col = i - row * TX;
    const int lx = col + R;
    uint8_t h0 = NONE, h1 = NONE;
    for (int dx = 0; dx <= R; ++dx) {
      const uint8_t l = t[row][lx - dx], r = t[row][lx + dx];
      if (h0 == NONE && (l == 0 || r == 0)) h0 = (uint8_t)dx;
      if (h1 == NONE && (l == 1 || r == 1)) h1 = (uint8_t)dx;
    }
    hd[0][row][col] = h0;
    hd[1][row][col] = h1;
  }
  __syncthreads();
  const int gx = x0 + threadIdx.x, gy = y0 + threadIdx.y;
  if (gx < a.W && gy < a.H) {
    const int v = t[threadIdx.y + R][threadIdx.x + R];
    int d = R + 1;   // "none within R"
    for (int dy = -R; dy <= R; ++dy) {
      const int h = hd[1 - v][threadIdx.y + R + dy][threadIdx.x];
      if (h != NONE) d = min(d, max(dy < 0 ? -dy : dy, h));
    }
    const int c = d <= a.edge_step ? a.edge_step - d + 1 : 0;
    const size_t p = plane + (size_t)gy * a.W + gx;
    a.eroded[p] = (v == 1 && d > a.erode_radius) ? 1.0f : 0.0f;
    a.certainty[p] = (float)c;
    if (c > 0) atomicMax(&block_max, c);   // LDS, integers: order-free
  }
  __syncthreads();
  if (tid == 0) a.tile_max[(size_t)b * tiles_x * tiles_y + (size_t)blockIdx.y * tiles_x + blockIdx.x] = block_max;
}

__global__ __launch_bounds__(THREADS) void morph_finish_kernel(mli_label_morph_args a, int tiles) {
  __shared__ int part[THREADS];
  const int b = blockIdx.y;
  const int n = a.H * a.W;
  int m = 0;
  for (int i = threadIdx.x; i < tiles; i += THREADS) m = max(m, a.tile_max[(size_t)b * tiles + i]);
  part[threadIdx.x] = m;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] = max(part[threadIdx.x], part[threadIdx.x + s]);
    __syncthreads();
  }
  const int cmax = part[0];
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= n) return;
  const size_t p = (size_t)b * n + i;
  const float c = a.certainty[p];
  a.certainty[p] = cmax > 0 ? 1.0f - c / (float)cmax : 1.0f;
  if (a.normal_x_light != nullptr) {
    float ps = a.normal_x_light[p] * a.eroded[p];
    if (a.inter_mask != nullptr) ps = ps * a.inter_mask[p];
    a.shading[p] = ps;
    a.shading_gamma[p] = powf(ps, a.inv_gamma);
  }
}

// ------------------------------------------------------------------------------ k-means
struct Pt {
  float x, y;
};

MLI_FI Pt opp_point(const float* image, size_t n, int l, int p) {
  const float* q = image + (size_t)l * 3 * n + p;
  const float r = q[0], g = q[n], b = q[2 * n];
  Pt o;
  o.x = (r - g) / (float)1.4142135623730951;
  o.y = ((r + g) - 2.0f * b) / (float)2.449489742783178;
  return o;
}

MLI_FI float dist2(Pt a, float cx, float cy) {
  const float dx = a.x - cx, dy = a.y - cy;
  return dx * dx + dy * dy;
}

// nearest of the first K centres, lowest index on ties
MLI_FI int nearest(Pt x, const float (&cx)[KMAX], const float (&cy)[KMAX], int K) {
  int best = 0;
  float bd = dist2(x, cx[0], cy[0]);
#pragma unroll
  for (int j = 1; j < KMAX; ++j)
    if (j < K) {
      const float d = dist2(x, cx[j], cy[j]);
      if (d < bd) {
        bd = d;
        best = j;
      }
    }
  return best;
}

__global__ __launch_bounds__(THREADS) void kmeans_kernel(mli_label_kmeans_args a) {
  const int p = blockIdx.x * THREADS + threadIdx.x;
  if (p >= a.n_pixels) return;
  const size_t n = (size_t)a.n_pixels;
  const int L = a.L, K = a.K;
  float cx[KMAX], cy[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) cx[j] = cy[j] = 0.0f;
  {
    const Pt x0 = opp_point(a.image, n, 0, p);
    cx[0] = x0.x;
    cy[0] = x0.y;
  }
#pragma unroll
  for (int j = 1; j < KMAX; ++j)
    if (j < K) {   // the point farthest from the centres chosen so far
      float far = -1.0f;
      Pt pick = {0.0f, 0.0f};
      for (int l = 0; l < L; ++l) {
        const Pt x = opp_point(a.image, n, l, p);
        float m = dist2(x, cx[0], cy[0]);
#pragma unroll
        for (int i = 1; i < KMAX; ++i)
          if (i < j) m = fminf(m, dist2(x, cx[i], cy[i]));
        if (m > far) {
          far = m;
          pick = x;
        }
      }
      cx[j] = pick.x;
      cy[j] = pick.y;
    }
  int pass = 0;
  while (pass < a.max_iter) {
    float sx[KMAX], sy[KMAX];
    int cnt[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
      sx[j] = sy[j] = 0.0f;
      cnt[j] = 0;
    }
    bool changed = pass == 0;
    for (int l = 0; l < L; ++l) {
      const Pt x = opp_point(a.image, n, l, p);
      const int k = nearest(x, cx, cy, K);
      uint8_t* lab = a.labels + (size_t)l * n + p;
      if (pass > 0 && *lab != (uint8_t)k) changed = true;
      *lab = (uint8_t)k;
#pragma unroll
      for (int j = 0; j < KMAX; ++j)
        if (j == k) {
          sx[j] = sx[j] + x.x;
          sy[j] = sy[j] + x.y;
          cnt[j] += 1;
        }
    }
    ++pass;
    if (!changed) break;
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
      if (j < K && cnt[j] > 0) {
        cx[j] = sx[j] / (float)cnt[j];
        cy[j] = sy[j] / (float)cnt[j];
      }
  }
#pragma unroll
  for (int j = 0; j < KMAX; ++j)
    if (j < K) {
      a.centers[((size_t)j * 2 + 0) * n + p] = cx[j];
      a.centers[((size_t)j * 2 + 1) * n + p] = cy[j];
    }
  if (a.passes != nullptr) a.passes[p] = pass;
}

// ------------------------------------------------------------------------------ best reflectance
__global__ __launch_bounds__(THREADS) void best_ref_kernel(mli_label_best_ref_args a) {
  const int p = blockIdx.x * THREADS + threadIdx.x;
  if (p >= a.n_pixels) return;
  const size_t n = (size_t)a.n_pixels;
  const int L = a.L, K = a.K;
  int cnt[KMAX];
#pragma unroll
  for (int j = 0; j < KMAX; ++j) cnt[j] = 0;
  bool any = false;
  for (int l = 0; l < L; ++l) {
    const bool m = a.shading[(size_t)l * n + p] > a.threshold;
    any = any || m;
    const int k = a.labels[(size_t)l * n + p];
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
      if (m && j == k) cnt[j] += 1;
  }
  int cmax = 0;
#pragma unroll
  for (int j = 0; j < KMAX; ++j)
    if (j < K) cmax = max(cmax, cnt[j]);
  uint32_t winners = 0;
#pragma unroll
  for (int j = 0; j < KMAX; ++j)
    if (j < K && cnt[j] == cmax) winners |= 1u << j;
  float smax = -INFINITY;
  for (int l = 0; l < L; ++l) {
    const float ps = a.shading[(size_t)l * n + p];
    const int k = a.labels[(size_t)l * n + p];
    const bool g = ps > a.threshold && k < K && (winners >> k & 1u);
    smax = fmaxf(smax, ps * (g ? 1.0f : 0.0f));
  }
  const float bar = a.threshold_wrt_max * smax;
  float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
  int keep = 0;
  for (int l = 0; l < L; ++l) {
    const float ps = a.shading[(size_t)l * n + p];
    const int k = a.labels[(size_t)l * n + p];
    const bool g = ps > a.threshold && k < K && (winners >> k & 1u);
    if (g && ps > bar) {
      const float psg = a.shading_gamma[(size_t)l * n + p];
      const float* q = a.image + (size_t)l * 3 * n + p;
      s0 = s0 + q[0] / psg;
      s1 = s1 + q[n] / psg;
      s2 = s2 + q[2 * n] / psg;
      keep += 1;
    }
  }
  const float den = (float)max(keep, 1);
  a.average_ref[p] = s0 / den;
  a.average_ref[n + p] = s1 / den;
  a.average_ref[2 * n + p] = s2 / den;
  a.keep_count[p] = keep;
  a.any_mask[p] = any ? 1 : 0;
}

// ------------------------------------------------------------------------------ nearest-donor fill
constexpr int feat_stride(int K) { return (5 + 2 * K + 3) & ~3; }   // 8, 12, 12, 16 floats

__global__ __launch_bounds__(THREADS) void fill_feat_kernel(mli_label_fill_args a, const int32_t* idx, int count,
                                                            float* out, int FS) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= count) return;
  const int n = a.H * a.W;
  const int p = idx[i];
  float* f = out + (size_t)i * FS;
  if (p < 0 || p >= n) {   // not a pixel: never the nearest of anything
    for (int q = 0; q < FS; ++q) f[q] = NAN;
    return;
  }
  const int y = p / a.W, x = p - y * a.W;
  const float den = (float)max(max(a.H - 1, a.W - 1), 1);
  f[0] = (float)y / den * 4.0f;
  f[1] = (float)x / den * 4.0f;
  const float nx = a.normal[p], ny = a.normal[(size_t)n + p], nz = a.normal[2 * (size_t)n + p];
  const float norm = sqrtf((nx * nx + ny * ny) + nz * nz) + 1e-10f;
  f[2] = nx / norm;
  f[3] = ny / norm;
  f[4] = nz / norm;
  for (int j = 0; j < a.K; ++j) {
    f[5 + 2 * j] = a.centers[((size_t)j * 2 + 0) * n + p];
    f[6 + 2 * j] = a.centers[((size_t)j * 2 + 1) * n + p];
  }
  for (int q = 5 + 2 * a.K; q < FS; ++q) f[q] = 0.0f;
}

template <int K>
__global__ __launch_bounds__(THREADS) void fill_search_kernel(mli_label_fill_args a, int slices) {
  constexpr int FS = feat_stride(K), Q = FS / 4;
  __shared__ float4 tile[DTILE * Q];
  const int h = blockIdx.x * THREADS + threadIdx.x;
  const bool live = h < a.n_holes;
  float hf[FS];
  {
    const float4* src = reinterpret_cast<const float4*>(a.hole_feat) + (size_t)(live ? h : 0) * Q;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float4 v = src[q];
      hf[4 * q] = v.x, hf[4 * q + 1] = v.y, hf[4 * q + 2] = v.z, hf[4 * q + 3] = v.w;
    }
  }
  const int tiles = (a.n_donors + DTILE - 1) / DTILE;
  const int per = (tiles + slices - 1) / slices;
  const int t0 = min((int)blockIdx.y * per, tiles), t1 = min(t0 + per, tiles);
  float best = INFINITY;
  uint32_t best_i = 0xffffffffu;
  const float4* dsrc = reinterpret_cast<const float4*>(a.donor_feat);
  for (int t = t0; t < t1; ++t) {   // (uniform per workgroup)
    const int base = t * DTILE;
    const int cnt = min(DTILE, a.n_donors - base);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * Q; i += THREADS) tile[i] = dsrc[(size_t)base * Q + i];
    __syncthreads();
#pragma unroll 2
    for (int d = 0; d < cnt; ++d) {   // the same LDS address in every lane: a broadcast read
      float df[FS];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const float4 v = tile[d * Q + q];
        df[4 * q] = v.x, df[4 * q + 1] = v.y, df[4 * q + 2] = v.z, df[4 * q + 3] = v.w;
      }
      float D = 0.0f;
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        const float e = hf[q] - df[q];
        D = q == 0 ? e * e : D + e * e;
      }
      float cmin = INFINITY;
#pragma unroll
      for (int i = 0; i < K; ++i)
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const float ex = hf[5 + 2 * i] - df[5 + 2 * j], ey = hf[6 + 2 * i] - df[6 + 2 * j];
          cmin = fminf(cmin, ex * ex + ey * ey);
        }
      D = D + cmin;
      if (D < best) {   // ascending donor position: the lowest one wins a tie
        best = D;
        best_i = (uint32_t)(base + d);
      }
    }
  }
  if (live) a.partial[(size_t)blockIdx.y * a.n_holes + h] = (uint64_t)__float_as_uint(best) << 32 | best_i;
}

__global__ __launch_bounds__(THREADS) void fill_reduce_kernel(mli_label_fill_args a, int slices) {
  const int h = blockIdx.x * THREADS + threadIdx.x;
  if (h >= a.n_holes) return;
  // D >= 0: its bit pattern orders as the value does, so the packed minimum is the smallest D and,
  // among equals, the lowest donor position
  uint64_t m = ~0ull;
  for (int s = 0; s < slices; ++s) {
    const uint64_t v = a.partial[(size_t)s * a.n_holes + h];
    m = v < m ? v : m;
  }
  const uint32_t bi = (uint32_t)(m & 0xffffffffu);
  if (bi >= (uint32_t)a.n_donors) return;   // no finite distance: the hole stays as it is
  const int n = a.H * a.W;
  const int hp = a.hole_idx[h], dp = a.donor_idx[bi];
  if (hp < 0 || hp >= n || dp < 0 || dp >= n) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) a.ref[(size_t)c * n + hp] = a.ref[(size_t)c * n + dp];
}

// ------------------------------------------------------------------------------ host checks
bool side_ok(int H, int W) { return H >= 1 && W >= 1 && H <= MLI_LABELS_MAX_SIDE && W <= MLI_LABELS_MAX_SIDE; }
bool planes_ok(int n) { return n >= 1 && n <= MLI_LABELS_MAX_PLANES; }
bool k_ok(int K) { return K >= 1 && K <= MLI_LABELS_MAX_K; }
int blocks_of(int n) { return (n + THREADS - 1) / THREADS; }

bool morph_ok(const mli_label_morph_args* a) {
  return side_ok(a->H, a->W) && planes_ok(a->B) && a->erode_radius >= 0 && a->erode_radius <= RMAX &&
         a->edge_step >= 0 && a->edge_step <= RMAX;
}

bool pixels_ok(int L, int K, int n_pixels) {
  return planes_ok(L) && k_ok(K) && L >= K && n_pixels >= 1 &&
         (int64_t)n_pixels <= (int64_t)MLI_LABELS_MAX_SIDE * MLI_LABELS_MAX_SIDE;
}

// shape limits of mli_label_fill; the number of donor slices
bool fill_plan(const mli_label_fill_args* a, int* slices) {
  if (!side_ok(a->H, a->W) || !k_ok(a->K)) return false;
  const int64_t n = (int64_t)a->H * a->W;
  if (a->n_holes < 0 || a->n_donors < 1 || a->n_holes > n || a->n_donors > n) return false;
  if (a->slices < 0 || a->slices > MLI_LABELS_MAX_SLICES) return false;
  const int tiles = (a->n_donors + DTILE - 1) / DTILE;
  int s = a->slices;
  if (s == 0) {   // enough workgroups for 4 per CU, no slice without a tile
    const int bx = a->n_holes > 0 ? blocks_of(a->n_holes) : 1;
    s = (1024 + bx - 1) / bx;
    s = s < MLI_LABELS_MAX_SLICES ? s : MLI_LABELS_MAX_SLICES;
    s = s < tiles ? s : tiles;
  }
  *slices = s;
  return true;
}

template <int K>
void launch_search(const mli_label_fill_args& a, int slices, hipStream_t s) {
  hipLaunchKernelGGL(fill_search_kernel<K>, dim3(blocks_of(a.n_holes), slices), dim3(THREADS), 0, s, a, slices);
}

}  // namespace

extern "C" int mli_labels_abi_version(void) { return MLI_LABELS_ABI_VERSION; }

extern "C" int mli_label_morph_workspace(const mli_label_morph_args* a, int64_t* bytes) {
  if (!morph_ok(a)) return (int)hipErrorInvalidValue;
  const int64_t tiles = (int64_t)((a->W + TX - 1) / TX) * ((a->H + TY - 1) / TY);
  bytes[0] = (int64_t)a->B * tiles * sizeof(int32_t);
  return 0;
}

extern "C" int mli_label_morph(const mli_label_morph_args* a, mli_stream_t s) {
  if (!morph_ok(a)) return (int)hipErrorInvalidValue;
  if (a->visibility == nullptr || a->eroded == nullptr || a->certainty == nullptr || a->tile_max == nullptr)
    return (int)hipErrorInvalidValue;
  const bool shade = a->normal_x_light != nullptr;
  if (shade != (a->shading != nullptr) || shade != (a->shading_gamma != nullptr)) return (int)hipErrorInvalidValue;
  if (!shade && a->inter_mask != nullptr) return (int)hipErrorInvalidValue;
  const int tiles_x = (a->W + TX - 1) / TX, tiles_y = (a->H + TY - 1) / TY;
  hipLaunchKernelGGL(morph_tile_kernel, dim3(tiles_x, tiles_y, a->B), dim3(TX, TY), 0, (hipStream_t)s, *a, tiles_x,
                     tiles_y);
  hipLaunchKernelGGL(morph_finish_kernel, dim3(blocks_of(a->H * a->W), a->B), dim3(THREADS), 0, (hipStream_t)s, *a,
                     tiles_x * tiles_y);
  return (int)hipGetLastError();
}

extern "C" int mli_label_kmeans(const mli_label_kmeans_args* a, mli_stream_t s) {
  if (!pixels_ok(a->L, a->K, a->n_pixels) || a->max_iter < 1) return (int)hipErrorInvalidValue;
  if (a->image == nullptr || a->labels == nullptr || a->centers == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kmeans_kernel, dim3(blocks_of(a->n_pixels)), dim3(THREADS), 0, (hipStream_t)s, *a);
  return (int)hipGetLastError();
}

extern "C" int mli_label_best_ref(const mli_label_best_ref_args* a, mli_stream_t s) {
  if (!pixels_ok(a->L, a->K, a->n_pixels)) return (int)hipErrorInvalidValue;
  if (a->image == nullptr || a->shading == nullptr || a->shading_gamma == nullptr || a->labels == nullptr ||
      a->average_ref == nullptr || a->keep_count == nullptr || a->any_mask == nullptr)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(best_ref_kernel, dim3(blocks_of(a->n_pixels)), dim3(THREADS), 0, (hipStream_t)s, *a);
  return (int)hipGetLastError();
}

extern "C" int mli_label_fill_workspace(const mli_label_fill_args* a, int64_t* bytes) {
  int slices;
  if (!fill_plan(a, &slices)) return (int)hipErrorInvalidValue;
  const int64_t row = (int64_t)feat_stride(a->K) * sizeof(float);
  bytes[0] = (int64_t)a->n_holes * row;
  bytes[1] = (int64_t)a->n_donors * row;
  bytes[2] = (int64_t)slices * a->n_holes * sizeof(uint64_t);
  return 0;
}

extern "C" int mli_label_fill(const mli_label_fill_args* a, mli_stream_t s) {
  int slices;
  if (!fill_plan(a, &slices)) return (int)hipErrorInvalidValue;
  if (a->n_holes == 0) return 0;
  if (a->normal == nullptr || a->centers == nullptr || a->hole_idx == nullptr || a->donor_idx == nullptr ||
      a->ref == nullptr || a->hole_feat == nullptr || a->donor_feat == nullptr || a->partial == nullptr)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)a->hole_feat | (uintptr_t)a->donor_feat) & 15) return (int)hipErrorInvalidValue;  // 16 B rows
  const int FS = feat_stride(a->K);
  hipStream_t st = (hipStream_t)s;
  hipLaunchKernelGGL(fill_feat_kernel, dim3(blocks_of(a->n_holes)), dim3(THREADS), 0, st, *a, a->hole_idx,
                     a->n_holes, a->hole_feat, FS);
  hipLaunchKernelGGL(fill_feat_kernel, dim3(blocks_of(a->n_donors)), dim3(THREADS), 0, st, *a, a->donor_idx,
                     a->n_donors, a->donor_feat, FS);
  switch (a->K) {
    case 1: launch_search<1>(*a, slices, st); break;
    case 2: launch_search<2>(*a, slices, st); break;
    case 3: launch_search<3>(*a, slices, st); break;
    default: launch_search<4>(*a, slices, st); break;
  }
  hipLaunchKernelGGL(fill_reduce_kernel, dim3(blocks_of(a->n_holes)), dim3(THREADS), 0, st, *a, slices);
  return (int)hipGetLastError();
}
