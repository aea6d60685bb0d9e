// Image metrics (MSE, PSNR, SSIM) -- include/mli_metrics.h.
//
//   metrics_tile_kernel    one 32 x 8 pixel tile of one (image, channel) per workgroup.  The prepared
//                          prediction and target of the tile and its 3-pixel halo go to LDS as doubles
//                          (14 x 38 each, dense: consecutive lanes touch consecutive 8-byte words in
//                          every pass, so neither the 64-bank reads nor the 32-bank writes conflict);
//                          the five 7 x 7 window sums are formed separably (7 across, left to right,
//                          into LDS; then 7 down, top to bottom), S is evaluated for the window centres
//                          the tile owns and the squared error for the pixels it owns, and one
//                          (sum S, sum squared error) partial leaves the workgroup, reduced by a tree
//                          over the thread index
//   metrics_reduce_kernel  one workgroup per image: per channel, thread t adds the partials of the
//                          tiles t, t + 256, ... in ascending order, the 256 sums go through the same
//                          tree, thread 0 forms the outputs
// No atomics and no order that depends on the launch: the same input gives the same bits, and an
// image's bits do not depend on the batch around it.  A window sum is a function of its 49 pixels
// alone (the same additions in the same order wherever the tile boundaries fall).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mli_metrics.h"

#define MLI_FI __device__ __forceinline__

namespace {

constexpr int TX = MLI_METRICS_TILE_X, TY = MLI_METRICS_TILE_Y;
constexpr int WIN = MLI_METRICS_WINDOW, HALO = WIN / 2;
constexpr int THREADS = TX * TY;
constexpr int ROWS = TY + 2 * HALO;   // 14
constexpr int COLS = TX + 2 * HALO;   // 38
static_assert(THREADS == 256, "the reduction trees are written for 256 threads");

struct Partial {
  double s, e;
};

MLI_FI double load_pixel(const float* f, const uint8_t* u, size_t i, bool quantize) {
  if (u != nullptr) return (double)u[i] / 255.0;
  const float v = f[i];
  if (!quantize) return (double)v;
  const float c = fminf(fmaxf(v, 0.0f), 1.0f);
  return (double)(uint8_t)(c * 255.0f) / 255.0;   // save_image: mul(255).byte()
}

// the sum of red[0 .. 255] in red[0], in an order fixed by the thread index
MLI_FI void tree_sum(double* red_s, double* red_e, int tid) {
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red_s[tid] = red_s[tid] + red_s[tid + s];
      red_e[tid] = red_e[tid] + red_e[tid + s];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(THREADS) void metrics_tile_kernel(mli_image_metrics_args a, int tiles_x, int tiles_y) {
  __shared__ double xs[ROWS * COLS], ys[ROWS * COLS];
  __shared__ double hs[5][ROWS][TX];   // row sums of x, y, x*x, y*y, x*y; the reduction reuses it
  const int tid = threadIdx.y * TX + threadIdx.x;
  const int plane = blockIdx.z;        // b * C + c
  const int b = plane / a.C;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const size_t n = (size_t)a.H * a.W;
  const size_t poff = (size_t)plane * n, aoff = (size_t)b * n;
  const bool has_alpha = a.alpha_f32 != nullptr || a.alpha_u8 != nullptr;
  const bool quantize = a.quantize != 0;
  for (int i = tid; i < ROWS * COLS; i += THREADS) {
    const int ly = i / COLS, lx = i - ly * COLS;
    const int gy = y0 + ly - HALO, gx = x0 + lx - HALO;
    double p = 0.0, t = 0.0;   // outside the image: never under a valid centre
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const size_t q = (size_t)gy * a.W + gx;
      p = load_pixel(a.pred_f32, a.pred_u8, poff + q, quantize);
      t = load_pixel(a.target_f32, a.target_u8, poff + q, quantize);
      if (has_alpha) {
        const double al = a.alpha_u8 != nullptr ? (double)a.alpha_u8[aoff + q] / 255.0 : (double)a.alpha_f32[aoff + q];
        const double white = 1.0 * (1.0 - al);
        t = t * al + white;
        if (a.mask_pred) p = p * al + white;
      }
      if (a.gamma_target) t = pow(t, a.inv_gamma);
      if (ly >= HALO && ly < HALO + TY && lx >= HALO && lx < HALO + TX) {   // this tile owns the pixel
        if (a.prep_pred != nullptr) a.prep_pred[poff + q] = p;
        if (a.prep_target != nullptr) a.prep_target[poff + q] = t;
      }
    }
    xs[i] = p;
    ys[i] = t;
  }
  __syncthreads();
  for (int i = tid; i < ROWS * TX; i += THREADS) {
    const int r = i / TX, c = i - r * TX;
    const double* xr = xs + r * COLS + c;
    const double* yr = ys + r * COLS + c;
    double sx = xr[0], sy = yr[0], sxx = xr[0] * xr[0], syy = yr[0] * yr[0], sxy = xr[0] * yr[0];
#pragma unroll
    for (int k = 1; k < WIN; ++k) {
      const double x = xr[k], y = yr[k];
      sx = sx + x;
      sy = sy + y;
      sxx = sxx + x * x;
      syy = syy + y * y;
      sxy = sxy + x * y;
    }
    hs[0][r][c] = sx;
    hs[1][r][c] = sy;
    hs[2][r][c] = sxx;
    hs[3][r][c] = syy;
    hs[4][r][c] = sxy;
  }
  __syncthreads();
  const int gx = x0 + threadIdx.x, gy = y0 + threadIdx.y;
  double S = 0.0, se = 0.0;
  if (gy >= HALO && gy < a.H - HALO && gx >= HALO && gx < a.W - HALO) {   // a window centre
    double u[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      double s = hs[m][threadIdx.y][threadIdx.x];
#pragma unroll
      for (int k = 1; k < WIN; ++k) s = s + hs[m][threadIdx.y + k][threadIdx.x];
      u[m] = s / (double)(WIN * WIN);
    }
    constexpr double NP = WIN * WIN, COV = NP / (NP - 1.0);
    constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    const double ux = u[0], uy = u[1];
    const double vx = COV * (u[2] - ux * ux), vy = COV * (u[3] - uy * uy), vxy = COV * (u[4] - ux * uy);
    const double a1 = 2.0 * ux * uy + C1, a2 = 2.0 * vxy + C2;
    const double b1 = ux * ux + uy * uy + C1, b2 = vx + vy + C2;
    S = (a1 * a2) / (b1 * b2);
  }
  if (gy < a.H && gx < a.W) {
    const int i = (threadIdx.y + HALO) * COLS + threadIdx.x + HALO;
    const double d = xs[i] - ys[i];
    se = d * d;
  }
  __syncthreads();   // every read of hs is done
  double* red_s = &hs[0][0][0];
  double* red_e = red_s + THREADS;
  red_s[tid] = S;
  red_e[tid] = se;
  tree_sum(red_s, red_e, tid);
  if (tid == 0) {
    Partial* out = reinterpret_cast<Partial*>(a.partial);
    Partial v;
    v.s = red_s[0];
    v.e = red_e[0];
    out[((size_t)plane * tiles_y + blockIdx.y) * tiles_x + blockIdx.x] = v;
  }
}

__global__ __launch_bounds__(THREADS) void metrics_reduce_kernel(mli_image_metrics_args a, int tiles) {
  __shared__ double red_s[THREADS], red_e[THREADS];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const Partial* part = reinterpret_cast<const Partial*>(a.partial);
  const double centres = (double)(a.H - 2 * HALO) * (double)(a.W - 2 * HALO);
  double ssim_sum = 0.0, se_sum = 0.0;   // thread 0's
  for (int c = 0; c < a.C; ++c) {
    const Partial* p = part + ((size_t)b * a.C + c) * tiles;
    double s = 0.0, e = 0.0;
    for (int i = tid; i < tiles; i += THREADS) {
      s = s + p[i].s;
      e = e + p[i].e;
    }
    red_s[tid] = s;
    red_e[tid] = e;
    tree_sum(red_s, red_e, tid);
    if (tid == 0) {
      const double sc = red_s[0] / centres;
      a.ssim_channels[(size_t)b * a.C + c] = sc;
      ssim_sum = ssim_sum + sc;
      se_sum = se_sum + red_e[0];
    }
    __syncthreads();   // red_* are rewritten by the next channel
  }
  if (tid == 0) {
    const double mse = se_sum / ((double)a.C * (double)a.H * (double)a.W);
    a.mse[b] = mse;
    a.psnr[b] = mse == 0.0 ? (double)INFINITY : 10.0 * log10(1.0 / mse);
    a.ssim[b] = ssim_sum / (double)a.C;
  }
}

// ------------------------------------------------------------------------------ host checks
bool shape_ok(const mli_image_metrics_args* a) {
  return a->B >= 1 && a->B <= MLI_METRICS_MAX_IMAGES && a->C >= 1 && a->C <= MLI_METRICS_MAX_CHANNELS &&
         a->H >= WIN && a->W >= WIN && a->H <= MLI_METRICS_MAX_SIDE && a->W <= MLI_METRICS_MAX_SIDE;
}

int64_t tiles_of(const mli_image_metrics_args* a) {
  return (int64_t)((a->W + TX - 1) / TX) * ((a->H + TY - 1) / TY);
}

}  // namespace

extern "C" int mli_metrics_abi_version(void) { return MLI_METRICS_ABI_VERSION; }

extern "C" int mli_image_metrics_workspace(const mli_image_metrics_args* a, int64_t* bytes) {
  if (!shape_ok(a)) return (int)hipErrorInvalidValue;
  bytes[0] = (int64_t)a->B * a->C * tiles_of(a) * (int64_t)sizeof(Partial);
  return 0;
}

extern "C" int mli_image_metrics(const mli_image_metrics_args* a, mli_stream_t s) {
  if (!shape_ok(a)) return (int)hipErrorInvalidValue;
  if ((a->pred_f32 != nullptr) == (a->pred_u8 != nullptr)) return (int)hipErrorInvalidValue;
  if ((a->target_f32 != nullptr) == (a->target_u8 != nullptr)) return (int)hipErrorInvalidValue;
  if (a->alpha_f32 != nullptr && a->alpha_u8 != nullptr) return (int)hipErrorInvalidValue;
  const bool has_alpha = a->alpha_f32 != nullptr || a->alpha_u8 != nullptr;
  if (a->mask_pred && !has_alpha) return (int)hipErrorInvalidValue;
  if (a->gamma_target && !(a->inv_gamma > 0.0)) return (int)hipErrorInvalidValue;
  if (a->mse == nullptr || a->psnr == nullptr || a->ssim == nullptr || a->ssim_channels == nullptr ||
      a->partial == nullptr)
    return (int)hipErrorInvalidValue;
  if ((uintptr_t)a->partial & 7) return (int)hipErrorInvalidValue;   // pairs of doubles
  const int tiles_x = (a->W + TX - 1) / TX, tiles_y = (a->H + TY - 1) / TY;
  hipLaunchKernelGGL(metrics_tile_kernel, dim3(tiles_x, tiles_y, a->B * a->C), dim3(TX, TY), 0, (hipStream_t)s, *a,
                     tiles_x, tiles_y);
  hipLaunchKernelGGL(metrics_reduce_kernel, dim3(a->B), dim3(THREADS), 0, (hipStream_t)s, *a, tiles_x * tiles_y);
  return (int)hipGetLastError();
}
