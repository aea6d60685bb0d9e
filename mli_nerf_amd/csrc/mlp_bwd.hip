// Heads backward dX chain (the shared heads machinery: mlp_core.h).
#include "mlp_core.h"

namespace {

template <bool NODZ3>
__global__ __launch_bounds__(GBwd::THREADS) void rgb_bwd_kernel(mli_rgb_bwd_args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  // live rays: a workgroup past the live tiles returns before any DMA or barrier
  // (nonzero tiles: past the padded list)
  if (a.n_live_tiles && (int)(blockIdx.x * GBwd::NW) >= *(a.wtile_list ? a.n_wtiles_pad : a.n_live_tiles)) return;
  if (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) >= GBwd::NW / 2) rgb_bwd_body<GBwd, STORE, NODZ3>(a, lds);
  else rgb_bwd_body<GBwd, DMA, NODZ3>(a, lds);
}


}  // namespace

extern "C" int mli_rgb_bwd(const mli_rgb_bwd_args* a, mli_stream_t s) {
  const int S = a->R * a->N;
  if (S % 256 != 0) return (int)hipErrorInvalidValue;
  // live rays: both arrays or none; a workgroup holds whole rays
  if ((a->tile_list != nullptr) != (a->n_live_tiles != nullptr)) return (int)hipErrorInvalidValue;
  if (a->tile_list && (a->N <= 0 || 256 % a->N != 0 || a->N % 32 != 0)) return (int)hipErrorInvalidValue;
  // nonzero tiles: both arrays or none, with the live rays only
  if ((a->wtile_list != nullptr) != (a->n_wtiles_pad != nullptr)) return (int)hipErrorInvalidValue;
  if (a->wtile_list && !a->tile_list) return (int)hipErrorInvalidValue;
  if (a->skip_dz3)
    hipLaunchKernelGGL(rgb_bwd_kernel<true>, dim3(S / GBwd::SAMPLES), dim3(GBwd::THREADS), GBwd::LDS_BWD,
                       (hipStream_t)s, *a);
  else
    hipLaunchKernelGGL(rgb_bwd_kernel<false>, dim3(S / GBwd::SAMPLES), dim3(GBwd::THREADS), GBwd::LDS_BWD,
                       (hipStream_t)s, *a);
  MLI_LAUNCH_CHECK();
}

extern "C" int mli_rgb_bwd_workspace(const mli_rgb_bwd_args* a, int64_t* bytes) {
  const int64_t S = (int64_t)a->R * a->N;
  if (S <= 0 || S % 256 != 0) return (int)hipErrorInvalidValue;
  bytes[0] = 3 * 4 * 256 * S * 2;  // dzT
  bytes[1] = 3 * S * 16 * 2;       // dz4T (one-k-step fragment images)
  return 0;
}

