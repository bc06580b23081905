// LPIPS(VGG) of the novel-view-synthesis evaluation: the passes around the VGG-16 trunk's split convolutions.
//
// Replaces, for evaluation/novel_view_synthesis_bench/calculate_metric.py, the reference's per-image call
// third_party_model/anysplat/src/evaluation/metrics.py:22-34 (lpips 0.1 `LPIPS(net="vgg")`, `forward(in0, in1, normalize=True)`).
// The 13 convolutions of the trunk are v3a_conv_split (fp32-equivalent, ReLU epilogue, pair in / pair out); this file holds what
// lies between them:
//   1. lpips_input_kernel   uint8 [N,H,W,3] (PNG bytes) or f32 [N,3,H,W] in [0,1], pred and gt -> ONE pair [2][2N][H][W][CinP]
//                           (frames [0,N) = pred, [N,2N) = gt), channels-last, padding channels zero.  fp32 with torch's rounding
//                           points: x = u / 255 (ToTensor), x = 2 x - 1 (normalize=True), x = (x - shift) / scale (ScalingLayer).
//   2. lpips_pool_kernel    nn.MaxPool2d(2, 2) (floor mode) on pairs: (hi, lo) compared lexicographically, the winning pair copied
//                           verbatim - exact, hi + lo of the output is the fp32 max of the window.
//   3. lpips_head_kernel    per pixel of one tapped layer: f = hi + lo (exact in fp32), f^ = f / (sqrt(sum_c f^2) + 1e-10),
//                           d = sum_c w[c] (f^0 - f^1)^2 (lpips normalize_tensor, NetLinLayer), all of it in fp64; one fp64 partial
//                           sum of d per workgroup.  lpips_reduce_kernel sums each pair's partials in the order of fixed_sum.h and writes
//                           the spatial mean (spatial_average), optionally added to what `out` holds (the sum over the five layers).
//
// Determinism: no atomics.  The head's tiling depends on (h, w, C) only - one workgroup row per pair, a fixed number of pixels per
// workgroup - so a pair's score is bit-identical run to run and whatever other pairs share the launch.  Swapping pred and gt swaps
// f^0 and f^1, which leaves (f^0 - f^1)^2 and both group reductions bitwise unchanged: LPIPS(a, b) == LPIPS(b, a) exactly, and
// identical images give exactly 0.
//
// Bounds (LPIPS section): all three kernels are single streaming passes, HBM-bound - every element is read once and
// written once (input, pool) or read once (head), with 16-byte accesses.
#include "common.h"
#include "fixed_sum.h"
#include "../../include/vist3a_hip.h"

// No contraction: 2 x - 1 and (x - shift) / scale are separate torch ops, each rounded to fp32.
#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int HEAD_STEPS = 16;   // pixel steps per head workgroup: THREADS / (C / 8) pixels each

__device__ __forceinline__ void split8(const float* v, u32x4& hi, u32x4& lo) {
  hi = pack_bf16x8(v);
  float h[8], r[8];
  unpack_bf16x8(hi, h);
#pragma unroll
  for (int e = 0; e < 8; ++e) r[e] = v[e] - h[e];   // exact in fp32
  lo = pack_bf16x8(r);
}

struct InP {
  const void* pred;
  const void* gt;
  char* hi;
  char* lo;
  long HW;
  int N, f32_nchw, CinP;
};

// one thread = one pixel of one frame: 3 loads, CinP / 8 16-byte stores per plane
__global__ void __launch_bounds__(THREADS) lpips_input_kernel(InP p) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= p.HW) return;
  const int f = blockIdx.y;
  const int n = f < p.N ? f : f - p.N;
  const void* src = f < p.N ? p.pred : p.gt;
  float x[3];
  if (p.f32_nchw) {
    const float* s = (const float*)src + (size_t)n * 3 * p.HW + i;
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = s[(size_t)c * p.HW];
  } else {
    const unsigned char* s = (const unsigned char*)src + ((size_t)n * p.HW + i) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = (float)s[c] / 255.0f;   // ToTensor: float(u8).div(255)
  }
  // lpips ScalingLayer: torch.Tensor([-.030, -.088, -.188]) / ([.458, .448, .450]), fp32
  const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t = 2.0f * x[c] - 1.0f;
    v[c] = (t - shift[c]) / scale[c];
  }
  u32x4 h, l;
  split8(v, h, l);
  const size_t o = ((size_t)f * p.HW + i) * p.CinP * 2;   // bytes
  *(u32x4*)(p.hi + o) = h;
  *(u32x4*)(p.lo + o) = l;
  if (p.CinP == 16) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    *(u32x4*)(p.hi + o + 16) = z;
    *(u32x4*)(p.lo + o + 16) = z;
  }
}

struct PoolP {
  const char* xh;
  const char* xl;
  char* yh;
  char* yl;
  long total;   // F * oH * oW * C / 8
  int H, W, oH, oW, C8;
};

// one thread = 8 channels of one output pixel: 4 x 2 16-byte loads, 2 16-byte stores
__global__ void __launch_bounds__(THREADS) lpips_pool_kernel(PoolP p) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= p.total) return;
  const int c8 = (int)(i % p.C8);
  const long pix = i / p.C8;
  const int ox = (int)(pix % p.oW), oy = (int)((pix / p.oW) % p.oH);
  const long f = pix / ((long)p.oW * p.oH);
  const int C = p.C8 * 8;
  float bh[8], bl[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t e = (((size_t)f * p.H + 2 * oy + (k >> 1)) * p.W + 2 * ox + (k & 1)) * C + (size_t)c8 * 8;
    float h[8], l[8];
    unpack_bf16x8(*(const u32x4*)(p.xh + e * 2), h);
    unpack_bf16x8(*(const u32x4*)(p.xl + e * 2), l);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (k == 0 || h[j] > bh[j] || (h[j] == bh[j] && l[j] > bl[j])) {
        bh[j] = h[j];
        bl[j] = l[j];
      }
    }
  }
  // bf16 values re-packed: the conversion of an exact bf16 value is that value
  const size_t o = (size_t)i * 16;
  *(u32x4*)(p.yh + o) = pack_bf16x8(bh);
  *(u32x4*)(p.yl + o) = pack_bf16x8(bl);
}

struct HeadP {
  const char* xh;   // [2N][HW][C] hi plane
  const char* xl;   // lo plane
  const float* w;   // [C]
  double* part;     // [N][tiles]
  long HW;
  int N, C, tiles, tile_pix;
};

// sum over the G lanes of a pixel group (xor butterfly: every lane ends with the same, order-fixed value)
template <int G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
  for (int m = G / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// G = C / 8 lanes per pixel, each holding 8 channels of pred and gt in registers; THREADS / G pixels per step
template <int G>
__global__ void __launch_bounds__(THREADS) lpips_head_kernel(HeadP p) {
  __shared__ double red[THREADS];
  constexpr int PPB = THREADS / G;
  const int tid = threadIdx.x, g = tid % G, slot = tid / G;
  const int tile = blockIdx.x, n = blockIdx.y;
  const int C = p.C;
  float wv[8];
  {
    const f32x4 a = *(const f32x4*)(p.w + g * 8), b = *(const f32x4*)(p.w + g * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { wv[e] = a[e]; wv[4 + e] = b[e]; }
  }
  const long pix0 = (long)tile * p.tile_pix;
  const size_t f0 = (size_t)n * p.HW, f1 = (size_t)(p.N + n) * p.HW;
  double acc = 0.0;
  for (int k = slot; k < p.tile_pix; k += PPB) {   // the same trip count for every lane: the group sums need all lanes
    const long px = pix0 + k;
    const bool ok = px < p.HW;
    float a[8], b[8];
    if (ok) {
      const size_t ea = ((f0 + px) * C + g * 8) * 2, eb = ((f1 + px) * C + g * 8) * 2;
      float ah[8], al[8], bh[8], bl[8];
      unpack_bf16x8(*(const u32x4*)(p.xh + ea), ah);
      unpack_bf16x8(*(const u32x4*)(p.xl + ea), al);
      unpack_bf16x8(*(const u32x4*)(p.xh + eb), bh);
      unpack_bf16x8(*(const u32x4*)(p.xl + eb), bl);
#pragma unroll
      for (int e = 0; e < 8; ++e) { a[e] = ah[e] + al[e]; b[e] = bh[e] + bl[e]; }   // exact: the pair's fp32 value
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = b[e] = 0.f;
    }
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sa += (double)a[e] * (double)a[e];   // products exact in fp64
      sb += (double)b[e] * (double)b[e];
    }
    sa = group_sum<G>(sa);
    sb = group_sum<G>(sb);
    const double na = sqrt(sa) + 1e-10, nb = sqrt(sb) + 1e-10;
    double d = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const double t = (double)a[e] / na - (double)b[e] / nb;
      d += (double)wv[e] * (t * t);
    }
    d = group_sum<G>(d);
    if (ok && g == 0) acc += d;
  }
  const double s = block_sum<THREADS>(acc, red);
  if (tid == 0) p.part[(size_t)n * p.tiles + tile] = s;
}

__global__ void __launch_bounds__(THREADS) lpips_reduce_kernel(const double* part, int tiles, double inv_hw, double* out, int accumulate) {
  __shared__ double red[THREADS];
  const int n = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int t = tid; t < tiles; t += THREADS) s += part[(size_t)n * tiles + t];
  s = block_sum<THREADS>(s, red);
  if (tid == 0) {
    const double m = s * inv_hw;
    out[n] = accumulate ? out[n] + m : m;
  }
}

int head_group(int C) {   // lanes per pixel, 0 = channel count not taken
  if (C < 8 || C > 512 || C % 8) return 0;
  const int g = C / 8;
  return (g & (g - 1)) ? 0 : g;
}

int head_tile_pix(int C) { return HEAD_STEPS * (THREADS / head_group(C)); }

long head_tiles(long HW, int C) { return (HW + head_tile_pix(C) - 1) / head_tile_pix(C); }

bool head_bad(int N, int h, int w, int C) {
  return N < 1 || h < 1 || w < 1 || (long)h * w > 0x7fffffffL || !head_group(C);
}

}  // namespace

extern "C" int v3a_lpips_input(const void* pred, const void* gt, int f32_nchw, int N, int H, int W, int CinP, void* y_hi, void* y_lo,
                               void* stream) {
  if (!pred || !gt || !y_hi || !y_lo) return V3A_ERR_ARG;
  if (N < 1 || 2L * N > 65535 || H < 1 || W < 1 || (long)H * W > 0x7fffffffL || (CinP != 8 && CinP != 16)) return V3A_ERR_SHAPE;
  InP p{pred, gt, (char*)y_hi, (char*)y_lo, (long)H * W, N, f32_nchw ? 1 : 0, CinP};
  hipLaunchKernelGGL(lpips_input_kernel, dim3((unsigned)((p.HW + THREADS - 1) / THREADS), 2 * N), dim3(THREADS), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_lpips_pool(const void* x_hi, const void* x_lo, void* y_hi, void* y_lo, int F, int H, int W, int C, void* stream) {
  if (!x_hi || !x_lo || !y_hi || !y_lo) return V3A_ERR_ARG;
  if (F < 1 || H < 2 || W < 2 || C < 8 || C % 8) return V3A_ERR_SHAPE;
  PoolP p{(const char*)x_hi, (const char*)x_lo, (char*)y_hi, (char*)y_lo, (long)F * (H / 2) * (W / 2) * (C / 8), H, W, H / 2, W / 2, C / 8};
  const long blocks = (p.total + THREADS - 1) / THREADS;
  if (blocks > 0x7fffffffL) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(lpips_pool_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" long v3a_lpips_head_workspace_bytes(int N, int h, int w, int C) {
  if (head_bad(N, h, w, C)) return V3A_ERR_SHAPE;
  return (long)N * head_tiles((long)h * w, C) * (long)sizeof(double);
}

extern "C" int v3a_lpips_head(const void* x_hi, const void* x_lo, const float* weight, int N, int h, int w, int C, double* out,
                              int accumulate, void* workspace, long workspace_bytes, void* stream) {
  if (!x_hi || !x_lo || !weight || !out) return V3A_ERR_ARG;
  if (head_bad(N, h, w, C) || N > 65535) return V3A_ERR_SHAPE;
  const long need = v3a_lpips_head_workspace_bytes(N, h, w, C);
  if (!workspace || workspace_bytes < need) return V3A_ERR_WORKSPACE;
  HeadP p{(const char*)x_hi, (const char*)x_lo, weight, (double*)workspace, (long)h * w, N, C, (int)head_tiles((long)h * w, C), head_tile_pix(C)};
  const dim3 grid(p.tiles, N);
  switch (head_group(C)) {
    case 1: hipLaunchKernelGGL(lpips_head_kernel<1>, grid, dim3(THREADS), 0, (hipStream_t)stream, p); break;
    case 2: hipLaunchKernelGGL(lpips_head_kernel<2>, grid, dim3(THREADS), 0, (hipStream_t)stream, p); break;
    case 4: hipLaunchKernelGGL(lpips_head_kernel<4>, grid, dim3(THREADS), 0, (hipStream_t)stream, p); break;
    case 8: hipLaunchKernelGGL(lpips_head_kernel<8>, grid, dim3(THREADS), 0, (hipStream_t)stream, p); break;
    case 16: hipLaunchKernelGGL(lpips_head_kernel<16>, grid, dim3(THREADS), 0, (hipStream_t)stream, p); break;
    case 32: hipLaunchKernelGGL(lpips_head_kernel<32>, grid, dim3(THREADS), 0, (hipStream_t)stream, p); break;
    default: hipLaunchKernelGGL(lpips_head_kernel<64>, grid, dim3(THREADS), 0, (hipStream_t)stream, p); break;
  }
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(lpips_reduce_kernel, dim3(N), dim3(THREADS), 0, (hipStream_t)stream, p.part, p.tiles, 1.0 / (double)p.HW, out,
                     accumulate ? 1 : 0);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
