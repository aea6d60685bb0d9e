// LPIPS v0.1 / AlexNet -- include/mli_lpips.h.
//
//   lpips_pack_w_kernel     OIHW fp32 weights -> [K][Cout], K ordered (kh, kw, ci), zero rows past K
//   lpips_pack_small_kernel biases, lin vectors, shift and scale behind the weights
//   lpips_conv_kernel       implicit GEMM in exact fp32 on v_mfma_f32_32x32x2_f32.  M = the output
//                           pixels of all 2B images flattened, N = Cout, K = Cin*k*k.  A workgroup of
//                           4 waves owns a 64 x 64 tile of the output, each wave a 32 x 32 quarter; K
//                           advances 16 at a time through LDS.  Both LDS tiles are k-major with a row
//                           stride of 96 words: a wave's MFMA operand read takes 32 consecutive words
//                           of row k (lanes 0..31) and of row k+1 (lanes 32..63), which the stride puts
//                           on the other 32 banks; the A store is one word per lane along a row, the B
//                           store one aligned float4 per lane.  The next stage's global loads are
//                           issued before the MFMAs of the current one.  Every layer's Cin but the
//                           first is a multiple of 16, so a stage lies inside one filter tap and row m
//                           of A is 16 contiguous channels of one input pixel (zero outside the image).
//                           Layer 1 gathers element by element from the planar inputs and applies the
//                           scaling on the way; its K = 363 is padded to 368 with zero weights.
//                           An output element is one accumulator element from start to end: the same
//                           fmaf chain over k wherever its tile falls, so its bits depend on neither
//                           the batch nor the position of its image in it.  Epilogue: + bias, ReLU,
//                           channel-last store (32 consecutive channels per accumulator register).
//   lpips_pool_kernel       3 x 3 stride-2 max-pool, channel-last, a float4 of channels per thread
//   lpips_input_kernel      the scaled input as taps[0] (only when the taps are asked for)
//   lpips_dist_kernel       one workgroup per 16 tap pixels of one pair: a wave per pixel, the lanes
//                           over the channels, all in double; one partial per workgroup
//   lpips_reduce_kernel     one workgroup per pair: per layer, thread t adds the partials t, t + 256,
//                           ... in ascending order, a tree over the thread index, thread 0 divides
//                           and adds the five layers in order
// No atomics and no order that depends on the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mli_lpips.h"

#define MLI_FI __device__ __forceinline__

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NL = MLI_LPIPS_LAYERS;
constexpr int BM = MLI_LPIPS_TILE_M, BN = MLI_LPIPS_TILE_N, BK = MLI_LPIPS_TILE_K;
constexpr int LDS_STRIDE = 96;   // words per k row: 64 used, the next row 32 banks further
constexpr int THREADS = 256;
constexpr int DIST_PIX = MLI_LPIPS_DIST_PIXELS;
static_assert(BM == 64 && BN == 64 && BK == 16 && THREADS == 256, "the loader roles are written for these");
static_assert(DIST_PIX == 16, "4 waves x 4 pixels");

struct LayerDef {
  int cin, cout, ks, stride, pad;
};
constexpr LayerDef LAYER[NL] = {{3, 64, 11, 4, 2}, {64, 192, 5, 1, 2}, {192, 384, 3, 1, 1}, {384, 256, 3, 1, 1},
                                {256, 256, 3, 1, 1}};
constexpr int K1 = 3 * 11 * 11;
static_assert(MLI_LPIPS_K1_PADDED % BK == 0 && MLI_LPIPS_K1_PADDED >= K1 && MLI_LPIPS_K1_PADDED - K1 < BK, "K1 padding");

__host__ __device__ constexpr int cout_of(int l) { return l == 0 ? 64 : l == 1 ? 192 : l == 2 ? 384 : 256; }
constexpr int k_of(int l) { return LAYER[l].cin * LAYER[l].ks * LAYER[l].ks; }
constexpr int kpad_of(int l) { return l == 0 ? MLI_LPIPS_K1_PADDED : k_of(l); }

// offsets (floats) into the packed buffer
struct PackedLayout {
  int64_t w[NL], b[NL], lin[NL], shift, scale, total;
};

PackedLayout packed_layout() {
  PackedLayout p;
  int64_t o = 0;
  for (int l = 0; l < NL; ++l) {
    p.w[l] = o;
    o += (int64_t)kpad_of(l) * LAYER[l].cout;
  }
  for (int l = 0; l < NL; ++l) {
    p.b[l] = o;
    o += LAYER[l].cout;
  }
  for (int l = 0; l < NL; ++l) {
    p.lin[l] = o;
    o += LAYER[l].cout;
  }
  p.shift = o;
  p.scale = o + 4;
  p.total = o + 8;
  return p;
}

// ------------------------------------------------------------------------------ pack
__global__ __launch_bounds__(THREADS) void lpips_pack_w_kernel(const float* w, float* out, int cin, int cout, int ks,
                                                                int kpad) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= kpad * cout) return;
  const int k = i / cout, co = i - k * cout;
  float v = 0.0f;
  if (k < cin * ks * ks) {
    const int tap = k / cin, ci = k - tap * cin;
    const int kh = tap / ks, kw = tap - kh * ks;
    v = w[(((size_t)co * cin + ci) * ks + kh) * ks + kw];
  }
  out[i] = v;
}

__global__ __launch_bounds__(THREADS) void lpips_pack_small_kernel(mli_lpips_pack_args a, PackedLayout p) {
  const int t = threadIdx.x;
  const int l = blockIdx.x;
  if (l < NL) {
    for (int c = t; c < cout_of(l); c += THREADS) {
      a.packed[p.b[l] + c] = a.b[l][c];
      a.packed[p.lin[l] + c] = a.lin[l][c];
    }
  } else if (t < 8) {
    const int c = t & 3;
    const float v = c == 3 ? 0.0f : (t < 4 ? a.shift[c] : a.scale[c]);
    a.packed[(t < 4 ? p.shift : p.scale) + c] = v;
  }
}

// ------------------------------------------------------------------------------ input
struct InputDesc {
  const float* pred_f32;
  const uint8_t* pred_u8;
  const float* target_f32;
  const uint8_t* target_u8;
  const float* shift;
  const float* scale;
  int B, H, W, normalize;
};

// step 1 of the definition for channel c of pixel pix (y*W + x) of image img (>= B: a target)
MLI_FI float scaled_input(const InputDesc& d, int img, int c, size_t pix) {
  const bool tgt = img >= d.B;
  const size_t i = ((size_t)(tgt ? img - d.B : img) * 3 + c) * ((size_t)d.H * d.W) + pix;
  const float* f = tgt ? d.target_f32 : d.pred_f32;
  const uint8_t* u = tgt ? d.target_u8 : d.pred_u8;
  float v = f != nullptr ? f[i] : (float)((double)u[i] / 255.0);
  if (d.normalize) v = 2.0f * v - 1.0f;
  return (v - d.shift[c]) / d.scale[c];
}

__global__ __launch_bounds__(THREADS) void lpips_input_kernel(InputDesc d, float* out, size_t total) {
  const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (i >= total) return;
  const size_t q = i / 3;   // img * H*W + pix
  const int c = (int)(i - q * 3);
  const size_t hw = (size_t)d.H * d.W;
  const int img = (int)(q / hw);
  out[i] = scaled_input(d, img, c, q - (size_t)img * hw);
}

// ------------------------------------------------------------------------------ convolution
struct ConvParams {
  InputDesc src;     // layer 1
  const float* in;   // the other layers: channel-last [N][IH][IW][Cin]
  const float* w;    // [K][Cout]
  const float* bias; // [Cout]
  float* out;        // channel-last [N][OH][OW][Cout] = [M][Cout]
  int IH, IW, Cin, OH, OW, Cout, ks, stride, pad, K, M;
};

template <bool FIRST>
__global__ __launch_bounds__(THREADS) void lpips_conv_kernel(ConvParams p) {
  __shared__ float As[BK * LDS_STRIDE];
  __shared__ float Bs[BK * LDS_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  // loader roles: A row am, k quad akq (4 consecutive k); B row bk, 4 consecutive channels from bn
  const int am = tid & 63, akq = tid >> 6;
  const int bk = tid >> 4, bn = (tid & 15) * 4;
  const int m = m0 + am;
  const bool mvalid = m < p.M;
  int img = 0, oy = 0, ox = 0;
  if (mvalid) {
    const int per = p.OH * p.OW;
    img = m / per;
    const int r = m - img * per;
    oy = r / p.OW;
    ox = r - oy * p.OW;
  }
  const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
  const int chunks = p.K / BK;
  float ra[4];
  float4 rb;
  auto load = [&](int c) {
    rb = *reinterpret_cast<const float4*>(p.w + (size_t)(c * BK + bk) * p.Cout + n0 + bn);
    ra[0] = ra[1] = ra[2] = ra[3] = 0.0f;
    if (FIRST) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = c * BK + akq * 4 + j;
        if (mvalid && k < K1) {
          const int tap = k / 3, ci = k - tap * 3;
          const int kh = tap / 11, kw = tap - kh * 11;
          const int iy = iy0 + kh, ix = ix0 + kw;
          if (iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW) ra[j] = scaled_input(p.src, img, ci, (size_t)iy * p.IW + ix);
        }
      }
    } else {
      const int k0 = c * BK;
      const int tap = k0 / p.Cin, ci0 = k0 - tap * p.Cin;
      const int kh = tap / p.ks, kw = tap - kh * p.ks;
      const int iy = iy0 + kh, ix = ix0 + kw;
      if (mvalid && iy >= 0 && iy < p.IH && ix >= 0 && ix < p.IW) {
        const float4 v = *reinterpret_cast<const float4*>(
            p.in + (((size_t)img * p.IH + iy) * p.IW + ix) * p.Cin + ci0 + akq * 4);
        ra[0] = v.x;
        ra[1] = v.y;
        ra[2] = v.z;
        ra[3] = v.w;
      }
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  const int half = lane >> 5, l31 = lane & 31;
  load(0);
  for (int c = 0; c < chunks; ++c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) As[(akq * 4 + j) * LDS_STRIDE + am] = ra[j];
    *reinterpret_cast<float4*>(&Bs[bk * LDS_STRIDE + bn]) = rb;
    __syncthreads();
    if (c + 1 < chunks) load(c + 1);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const float av = As[(kk + half) * LDS_STRIDE + wm * 32 + l31];
      const float bv = Bs[(kk + half) * LDS_STRIDE + wn * 32 + l31];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  const int n = n0 + wn * 32 + l31;
  const float bias = p.bias[n];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
    const int mm = m0 + wm * 32 + row;
    if (mm < p.M) p.out[(size_t)mm * p.Cout + n] = fmaxf(acc[r] + bias, 0.0f);
  }
}

// ------------------------------------------------------------------------------ max-pool
__global__ __launch_bounds__(THREADS) void lpips_pool_kernel(const float* in, float* out, int IH, int IW, int C, int OH,
                                                              int OW, size_t total) {
  const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;   // (img, oy, ox, channel quad)
  if (i >= total) return;
  const int c4 = C >> 2;
  const size_t q = i / c4;
  const int cq = (int)(i - q * c4);
  const size_t per = (size_t)OH * OW;
  const size_t img = q / per;
  const int r = (int)(q - img * per);
  const int oy = r / OW, ox = r - oy * OW;
  const float* base = in + ((img * IH + (size_t)oy * 2) * IW + (size_t)ox * 2) * C + cq * 4;
  float4 v = *reinterpret_cast<const float4*>(base);
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float4 u = *reinterpret_cast<const float4*>(base + ((size_t)dy * IW + dx) * C);
      v.x = fmaxf(v.x, u.x);
      v.y = fmaxf(v.y, u.y);
      v.z = fmaxf(v.z, u.z);
      v.w = fmaxf(v.w, u.w);
    }
  *reinterpret_cast<float4*>(out + i * 4) = v;
}

// ------------------------------------------------------------------------------ distance
MLI_FI double wave_sum(double v) {   // a butterfly: every lane ends with the same bits
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = v + __shfl_xor(v, s, 64);
  return v;
}

__global__ __launch_bounds__(THREADS) void lpips_dist_kernel(const float* tap, const float* lin, int B, int npix, int C,
                                                              double* partial, int pair_stride) {
  __shared__ double ws[THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y;
  double wsum = 0.0;
  for (int q = 0; q < DIST_PIX / 4; ++q) {
    const int pix = blockIdx.x * DIST_PIX + wave * (DIST_PIX / 4) + q;   // the same for the whole wave
    if (pix >= npix) break;
    const float* x = tap + ((size_t)b * npix + pix) * C;
    const float* y = tap + ((size_t)(B + b) * npix + pix) * C;
    double sx = 0.0, sy = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double xv = (double)x[c], yv = (double)y[c];
      sx = sx + xv * xv;
      sy = sy + yv * yv;
    }
    const double nx = sqrt(wave_sum(sx)) + 1e-10, ny = sqrt(wave_sum(sy)) + 1e-10;
    double d = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double t = (double)x[c] / nx - (double)y[c] / ny;
      d = d + (double)lin[c] * (t * t);
    }
    wsum = wsum + wave_sum(d);
  }
  if (lane == 0) ws[wave] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) partial[(size_t)b * pair_stride + blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

struct ReduceDesc {
  int chunks[NL], offset[NL], npix[NL], pair_stride;
};

__global__ __launch_bounds__(THREADS) void lpips_reduce_kernel(const double* partial, ReduceDesc r, double* layers,
                                                                double* lpips) {
  __shared__ double red[THREADS];
  const int tid = threadIdx.x, b = blockIdx.x;
  double total = 0.0;   // thread 0's
  for (int l = 0; l < NL; ++l) {
    const double* p = partial + (size_t)b * r.pair_stride + r.offset[l];
    double s = 0.0;
    for (int i = tid; i < r.chunks[l]; i += THREADS) s = s + p[i];
    red[tid] = s;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
      if (tid < h) red[tid] = red[tid] + red[tid + h];
      __syncthreads();
    }
    if (tid == 0) {
      const double v = red[0] / (double)r.npix[l];
      layers[(size_t)b * NL + l] = v;
      total = total + v;
    }
    __syncthreads();   // red is rewritten by the next layer
  }
  if (tid == 0) lpips[b] = total;
}

// ------------------------------------------------------------------------------ host
struct Plan {
  int ih[NL], iw[NL];     // a convolution's input size
  int oh[NL], ow[NL];     // and its output (= the tap's) size
  int64_t conv[NL];       // scratch offsets (floats) of the convolution outputs
  int64_t pool[2];        // and of the two pool outputs
  int64_t partial;        // offset (bytes) of the partials
  ReduceDesc red;
  int64_t bytes;
};

bool shape_ok(const mli_lpips_args* a) {
  return a->B >= 1 && a->B <= MLI_LPIPS_MAX_PAIRS && a->H >= MLI_LPIPS_MIN_SIDE && a->W >= MLI_LPIPS_MIN_SIDE &&
         a->H <= MLI_LPIPS_MAX_SIDE && a->W <= MLI_LPIPS_MAX_SIDE;
}

int64_t align4(int64_t v) { return (v + 3) & ~(int64_t)3; }

Plan plan_of(const mli_lpips_args* a) {
  Plan p;
  const int64_t n = 2 * (int64_t)a->B;
  int h = a->H, w = a->W;
  int64_t o = 0;
  int stride = 0;
  for (int l = 0; l < NL; ++l) {
    if (l == 1 || l == 2) {   // the pool in front of layers 2 and 3
      h = (h - 3) / 2 + 1;
      w = (w - 3) / 2 + 1;
      p.pool[l - 1] = o;
      o += align4(n * h * w * LAYER[l].cin);
    }
    p.ih[l] = h;
    p.iw[l] = w;
    h = (h + 2 * LAYER[l].pad - LAYER[l].ks) / LAYER[l].stride + 1;
    w = (w + 2 * LAYER[l].pad - LAYER[l].ks) / LAYER[l].stride + 1;
    p.oh[l] = h;
    p.ow[l] = w;
    p.conv[l] = o;
    o += align4(n * h * w * LAYER[l].cout);
    p.red.npix[l] = h * w;
    p.red.chunks[l] = (h * w + DIST_PIX - 1) / DIST_PIX;
    p.red.offset[l] = stride;
    stride += p.red.chunks[l];
  }
  p.red.pair_stride = stride;
  p.partial = o * (int64_t)sizeof(float);   // a multiple of 16
  p.bytes = p.partial + (int64_t)a->B * stride * (int64_t)sizeof(double);
  return p;
}

unsigned blocks_of(size_t total) { return (unsigned)((total + THREADS - 1) / THREADS); }

}  // namespace

extern "C" int mli_lpips_abi_version(void) { return MLI_LPIPS_ABI_VERSION; }

extern "C" int mli_lpips_pack_workspace(const mli_lpips_pack_args* a, int64_t* bytes) {
  if (a == nullptr || bytes == nullptr) return (int)hipErrorInvalidValue;
  bytes[0] = packed_layout().total * (int64_t)sizeof(float);
  return 0;
}

extern "C" int mli_lpips_pack(const mli_lpips_pack_args* a, mli_stream_t s) {
  for (int l = 0; l < NL; ++l)
    if (a->w[l] == nullptr || a->b[l] == nullptr || a->lin[l] == nullptr) return (int)hipErrorInvalidValue;
  if (a->shift == nullptr || a->scale == nullptr || a->packed == nullptr) return (int)hipErrorInvalidValue;
  if ((uintptr_t)a->packed & 15) return (int)hipErrorInvalidValue;
  const PackedLayout p = packed_layout();
  for (int l = 0; l < NL; ++l) {
    const int total = kpad_of(l) * LAYER[l].cout;
    hipLaunchKernelGGL(lpips_pack_w_kernel, dim3(blocks_of(total)), dim3(THREADS), 0, (hipStream_t)s, a->w[l],
                       a->packed + p.w[l], LAYER[l].cin, LAYER[l].cout, LAYER[l].ks, kpad_of(l));
  }
  hipLaunchKernelGGL(lpips_pack_small_kernel, dim3(NL + 1), dim3(THREADS), 0, (hipStream_t)s, *a, p);
  return (int)hipGetLastError();
}

extern "C" int mli_lpips_workspace(const mli_lpips_args* a, int64_t* bytes) {
  if (!shape_ok(a)) return (int)hipErrorInvalidValue;
  bytes[0] = plan_of(a).bytes;
  return 0;
}

extern "C" int mli_lpips(const mli_lpips_args* a, mli_stream_t s) {
  if (!shape_ok(a)) return (int)hipErrorInvalidValue;
  if ((a->pred_f32 != nullptr) == (a->pred_u8 != nullptr)) return (int)hipErrorInvalidValue;
  if ((a->target_f32 != nullptr) == (a->target_u8 != nullptr)) return (int)hipErrorInvalidValue;
  if (a->packed == nullptr || a->lpips == nullptr || a->layers == nullptr || a->scratch == nullptr)
    return (int)hipErrorInvalidValue;
  if (((uintptr_t)a->packed & 15) || ((uintptr_t)a->scratch & 15)) return (int)hipErrorInvalidValue;
  int given = 0;
  for (int i = 0; i <= NL; ++i) {
    if (a->taps[i] != nullptr) ++given;
    if ((uintptr_t)a->taps[i] & 15) return (int)hipErrorInvalidValue;
  }
  if (given != 0 && given != NL + 1) return (int)hipErrorInvalidValue;
  const hipStream_t st = (hipStream_t)s;
  const Plan pl = plan_of(a);
  const PackedLayout pk = packed_layout();
  float* scratch = reinterpret_cast<float*>(a->scratch);
  const int n = 2 * a->B;
  InputDesc src;
  src.pred_f32 = a->pred_f32;
  src.pred_u8 = a->pred_u8;
  src.target_f32 = a->target_f32;
  src.target_u8 = a->target_u8;
  src.shift = a->packed + pk.shift;
  src.scale = a->packed + pk.scale;
  src.B = a->B;
  src.H = a->H;
  src.W = a->W;
  src.normalize = a->normalize != 0;
  if (given) {
    const size_t total = (size_t)n * a->H * a->W * 3;
    hipLaunchKernelGGL(lpips_input_kernel, dim3(blocks_of(total)), dim3(THREADS), 0, st, src, a->taps[0], total);
  }
  double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(a->scratch) + pl.partial);
  const float* prev = nullptr;   // the previous tap
  for (int l = 0; l < NL; ++l) {
    const float* in = prev;
    if (l == 1 || l == 2) {
      float* pooled = scratch + pl.pool[l - 1];
      const size_t total = (size_t)n * pl.ih[l] * pl.iw[l] * (LAYER[l].cin / 4);
      hipLaunchKernelGGL(lpips_pool_kernel, dim3(blocks_of(total)), dim3(THREADS), 0, st, prev, pooled, pl.oh[l - 1],
                         pl.ow[l - 1], LAYER[l].cin, pl.ih[l], pl.iw[l], total);
      in = pooled;
    }
    float* out = given ? a->taps[l + 1] : scratch + pl.conv[l];
    ConvParams c;
    c.src = src;
    c.in = in;
    c.w = a->packed + pk.w[l];
    c.bias = a->packed + pk.b[l];
    c.out = out;
    c.IH = pl.ih[l];
    c.IW = pl.iw[l];
    c.Cin = LAYER[l].cin;
    c.OH = pl.oh[l];
    c.OW = pl.ow[l];
    c.Cout = LAYER[l].cout;
    c.ks = LAYER[l].ks;
    c.stride = LAYER[l].stride;
    c.pad = LAYER[l].pad;
    c.K = kpad_of(l);
    c.M = n * pl.oh[l] * pl.ow[l];
    const dim3 grid((c.M + BM - 1) / BM, c.Cout / BN);
    if (l == 0)
      hipLaunchKernelGGL(lpips_conv_kernel<true>, grid, dim3(THREADS), 0, st, c);
    else
      hipLaunchKernelGGL(lpips_conv_kernel<false>, grid, dim3(THREADS), 0, st, c);
    hipLaunchKernelGGL(lpips_dist_kernel, dim3(pl.red.chunks[l], a->B), dim3(THREADS), 0, st, out,
                       a->packed + pk.lin[l], a->B, pl.red.npix[l], c.Cout, partial + pl.red.offset[l],
                       pl.red.pair_stride);
    prev = out;
  }
  hipLaunchKernelGGL(lpips_reduce_kernel, dim3(a->B), dim3(THREADS), 0, st, partial, pl.red, a->layers, a->lpips);
  return (int)hipGetLastError();
}
