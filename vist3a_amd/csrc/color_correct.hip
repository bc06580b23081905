// Colour correction of a render against its ground truth before PSNR (cc_psnr), and the plain per-image MSE of two f32 images.
// third_party_model/anysplat/src/post_opt/lib_bilagrid.py:56-126 (color_correct), used by simple_trainer.py::eval.
//
// Per image, RGB, K = num_iters rounds.  With x the current estimate (x = img before the first round, NOT clipped, as the reference):
//   features f(x) = (r^2, rg, rb, g^2, gb, b^2, r, g, b, 1)                         the order of the reference's a_mat
//   mask_c       = unclipped(img[c]) & unclipped(x[c]) & unclipped(ref[c]),  unclipped(z) = eps <= z <= 1 - eps
//   warp_c       = argmin_w sum_{mask_c} (f(x) . w - ref[c])^2                     10 coefficients per output channel
//   x            = clip(f(x) . warp, 0, 1)
// Everything after the f32 loads is fp64; the result is rounded to f32 once, on its only store.
//
// Launches: per round one accumulation and one solve, then one apply and one reduction (2 K + 2 in all); nothing is read back to
// the host in between.
//  accumulate  grid (B, 3, N), 256 threads.  One workgroup = one output channel of a slice of one image's pixels: a thread keeps that
//              channel's 55 Gram entries (upper triangle), 10 right-hand sides and the row count - 66 fp64 running sums, 132
//              VGPRs; all three channels in one thread would be 198 sums and spill.  The estimate x is NOT kept in memory between
//              rounds: every pass recomputes it from img through the warps of the earlier rounds (30 multiply-adds per round and
//              pixel, the warps staged in LDS), so x stays fp64 from the load to the store and `out` is written exactly once.
//              The workgroup's sums go through a fixed-order LDS tree into part[n][c][block][66].
//  solve       grid (3, N).  Adds the B partials of each sum in block order, then solves the 10 x 10 normal equations in fp64 in
//              LDS: elimination without row exchanges (the Gram matrix is symmetric positive semi-definite), the 10 x 11 augmented
//              entries one thread each, back-substitution on one thread.  The reference calls lstsq; for a full-rank system the
//              two agree to rounding (cond(Gram) = cond(A)^2, at fp64 far inside the f32 result for any image a metric is taken of).
//              RANK-DEFICIENT CHANNELS (a deviation: the reference asserts or is undefined there): with fewer than 10 rows used
//              (flag 1), or a pivot p_k <= 1e-12 G_kk of the untouched diagonal entry, or a non-finite solution (flag 2), the
//              channel's warp of this round is the identity (x[c] passes through, still clipped).  The flags of all rounds are
//              OR-ed into status[n][c].
//  apply       grid (B, N): x through all K warps, out = (float)x, and the squared difference of the STORED value to ref in fp64,
//              per workgroup (fixed_sum.h).
//  finish      grid (N): the B partials in block order -> sse[n]; status.
// B depends on H W alone (never on N), so an image's result does not depend on its neighbours in the call; no atomics anywhere:
// bit-identical run to run.
//
// v3a_image_mse: the same two-stage reduction over (a - b)^2 of f32 [N,H,W,C], the difference taken in fp64 (exact), -> mse[n].
//
// Layout: [N,H,W,3] with the pixel's channels contiguous; row stride ld_* and image stride *_stride in elements, so a crop or a
// slice of a larger buffer is read and written in place.  Only the [H, 3 W] region of each image is touched.
#include "common.h"
#include "fixed_sum.h"
#include "../../include/vist3a_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 128;        // workgroups per image (and channel)
constexpr int MAX_ITERS = 16;
constexpr int NF = 10;                 // features
constexpr int NS = 66;                 // 55 Gram + 10 right-hand sides + 1 count
constexpr int BATCH = 11;              // sums per pass of the LDS tree (6 passes)
constexpr int SOLVE_THREADS = 128;
constexpr double PIVOT_TOL = 1e-12;

struct CcP {
  const float* img; const float* ref; float* out;
  long ld_img, ld_ref, ld_out, img_stride, ref_stride, out_stride;
  int N, H, W, K;
  double lo, hi;                       // eps, 1 - eps
  double* part;                        // [N][3][B][NS]
  double* warps;                       // [N][K][3][NF]
  double* part_sse;                    // [N][B]
  int* flags;                          // [N][K][3]
};

__device__ __forceinline__ void features(const double (&x)[3], double (&f)[NF]) {
  f[0] = x[0] * x[0]; f[1] = x[0] * x[1]; f[2] = x[0] * x[2];
  f[3] = x[1] * x[1]; f[4] = x[1] * x[2];
  f[5] = x[2] * x[2];
  f[6] = x[0]; f[7] = x[1]; f[8] = x[2];
  f[9] = 1.0;
}

// x <- clip(f(x) . warp_t, 0, 1) for the rounds t < rounds; wl = [rounds][3][NF] in LDS
__device__ __forceinline__ void apply_rounds(double (&x)[3], const double* wl, int rounds) {
  for (int t = 0; t < rounds; ++t) {
    double f[NF];
    features(x, f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < NF; ++q) s += f[q] * wl[(t * 3 + c) * NF + q];
      x[c] = fmin(fmax(s, 0.0), 1.0);
    }
  }
}

__device__ __forceinline__ double pick(const double (&x)[3], int c) { return c == 0 ? x[0] : (c == 1 ? x[1] : x[2]); }

__device__ __forceinline__ void stage_warps(const CcP& p, int n, int rounds, double* wl) {
  const double* src = p.warps + (long)n * p.K * 3 * NF;
  for (int q = threadIdx.x; q < rounds * 3 * NF; q += THREADS) wl[q] = src[q];
  __syncthreads();
}

__global__ void __launch_bounds__(THREADS) cc_accumulate_kernel(const CcP p, int it) {
  __shared__ double wl[MAX_ITERS * 3 * NF];
  __shared__ double red[BATCH][THREADS];
  const int t = threadIdx.x, c = blockIdx.y, n = blockIdx.z;
  stage_warps(p, n, it, wl);
  double acc[NS];
#pragma unroll
  for (int q = 0; q < NS; ++q) acc[q] = 0.0;
  const long n_px = (long)p.H * p.W, stride = (long)gridDim.x * THREADS;
  for (long px = (long)blockIdx.x * THREADS + t; px < n_px; px += stride) {
    const long i = px / p.W, j = px - i * p.W;
    const float* s = p.img + (long)n * p.img_stride + i * p.ld_img + 3 * j;
    const double x0[3] = {(double)s[0], (double)s[1], (double)s[2]};
    double x[3] = {x0[0], x0[1], x0[2]};
    apply_rounds(x, wl, it);
    const double b = (double)p.ref[(long)n * p.ref_stride + i * p.ld_ref + 3 * j + c];
    const double xc0 = pick(x0, c), xc = pick(x, c);
    const bool use = xc0 >= p.lo && xc0 <= p.hi && xc >= p.lo && xc <= p.hi && b >= p.lo && b <= p.hi;
    if (use) {
      double f[NF];
      features(x, f);
#pragma unroll
      for (int a = 0; a < NF; ++a) {
#pragma unroll
        for (int k = a; k < NF; ++k) acc[a * NF - a * (a - 1) / 2 + (k - a)] += f[a] * f[k];   // = tri(a, k), constant once unrolled
      }
#pragma unroll
      for (int a = 0; a < NF; ++a) acc[55 + a] += f[a] * b;
      acc[65] += 1.0;
    }
  }
  double* dst = p.part + (((long)n * 3 + c) * gridDim.x + blockIdx.x) * NS;
#pragma unroll
  for (int pass = 0; pass < NS / BATCH; ++pass) {
#pragma unroll
    for (int q = 0; q < BATCH; ++q) red[q][t] = acc[pass * BATCH + q];
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
      if (t < s) {
#pragma unroll
        for (int q = 0; q < BATCH; ++q) red[q][t] += red[q][t + s];
      }
      __syncthreads();
    }
    if (t < BATCH) dst[pass * BATCH + t] = red[t][0];
    __syncthreads();
  }
}

// index of Gram entry (a, b), a <= b, in the packed upper triangle
__device__ __forceinline__ int tri(int a, int b) { return a * NF - a * (a - 1) / 2 + (b - a); }

__global__ void __launch_bounds__(SOLVE_THREADS) cc_solve_kernel(const CcP p, int it, int blocks) {
  __shared__ double S[NS];
  __shared__ double G[NF][NF + 2];     // augmented [G | rhs], one spare column
  __shared__ double w[NF];
  __shared__ int fail;
  const int t = threadIdx.x, c = blockIdx.x, n = blockIdx.y;
  if (t < NS) {
    const double* src = p.part + ((long)n * 3 + c) * blocks * NS + t;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += src[(long)b * NS];
    S[t] = s;
  }
  __syncthreads();
  const int i = t / (NF + 1), j = t % (NF + 1);
  const bool cell = t < NF * (NF + 1);
  if (cell) G[i][j] = j < NF ? S[tri(i < j ? i : j, i < j ? j : i)] : S[55 + i];
  if (t == 0) fail = S[65] < (double)NF ? 1 : 0;
  __syncthreads();
  for (int k = 0; k < NF; ++k) {
    const double piv = G[k][k], d0 = S[tri(k, k)];
    if (t == 0 && !(d0 > 0.0 && piv > PIVOT_TOL * d0)) fail |= 2;
    // row k and column k are not written in step k: the reads below do not race with the writes
    if (cell && i > k && j > k) G[i][j] -= (G[i][k] / piv) * G[k][j];
    __syncthreads();
  }
  if (t == 0) {
    bool finite = true;
    for (int r = NF - 1; r >= 0; --r) {
      double s = G[r][NF];
      for (int q = r + 1; q < NF; ++q) s -= G[r][q] * w[q];
      const double v = s / G[r][r];
      w[r] = v;
      finite = finite && isfinite(v);
    }
    if (!finite) fail |= 2;
  }
  __syncthreads();
  if (t < NF) p.warps[(((long)n * p.K + it) * 3 + c) * NF + t] = fail ? (t == 6 + c ? 1.0 : 0.0) : w[t];
  if (t == 0) p.flags[((long)n * p.K + it) * 3 + c] = fail;
}

__global__ void __launch_bounds__(THREADS) cc_apply_kernel(const CcP p) {
  __shared__ double wl[MAX_ITERS * 3 * NF];
  __shared__ double red[THREADS];
  const int t = threadIdx.x, n = blockIdx.y;
  stage_warps(p, n, p.K, wl);
  double err = 0.0;
  const long n_px = (long)p.H * p.W, stride = (long)gridDim.x * THREADS;
  for (long px = (long)blockIdx.x * THREADS + t; px < n_px; px += stride) {
    const long i = px / p.W, j = px - i * p.W;
    const float* s = p.img + (long)n * p.img_stride + i * p.ld_img + 3 * j;
    const float* r = p.ref + (long)n * p.ref_stride + i * p.ld_ref + 3 * j;
    float* o = p.out + (long)n * p.out_stride + i * p.ld_out + 3 * j;
    double x[3] = {(double)s[0], (double)s[1], (double)s[2]};
    apply_rounds(x, wl, p.K);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = (float)x[c];
      o[c] = v;
      const double d = (double)v - (double)r[c];
      err += d * d;
    }
  }
  const double total = block_sum<THREADS>(err, red);
  if (t == 0) p.part_sse[(long)n * gridDim.x + blockIdx.x] = total;
}

__global__ void __launch_bounds__(64) cc_finish_kernel(const CcP p, int blocks, double* sse, int* status) {
  const int t = threadIdx.x, n = blockIdx.x;
  if (t == 0) {
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += p.part_sse[(long)n * blocks + b];
    sse[n] = s;
  }
  if (t < 3) {
    int f = 0;
    for (int k = 0; k < p.K; ++k) f |= p.flags[((long)n * p.K + k) * 3 + t];
    status[n * 3 + t] = f;
  }
}

struct MseP {
  const float* a; const float* b;
  long ld_a, ld_b, a_stride, b_stride;
  int N, H, W, C;
};

__global__ void __launch_bounds__(THREADS) mse_partial_kernel(const MseP p, double* part) {
  __shared__ double red[THREADS];
  const int t = threadIdx.x, n = blockIdx.y;
  const long row = (long)p.W * p.C, total = row * p.H, stride = (long)gridDim.x * THREADS;
  double err = 0.0;
  for (long e = (long)blockIdx.x * THREADS + t; e < total; e += stride) {
    const long i = e / row, j = e - i * row;
    const double d = (double)p.a[(long)n * p.a_stride + i * p.ld_a + j] - (double)p.b[(long)n * p.b_stride + i * p.ld_b + j];
    err += d * d;
  }
  const double s = block_sum<THREADS>(err, red);
  if (t == 0) part[(long)n * gridDim.x + blockIdx.x] = s;
}

__global__ void __launch_bounds__(64) mse_finish_kernel(const double* part, int blocks, double count, double* mse) {
  if (threadIdx.x == 0) {
    const int n = blockIdx.x;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part[(long)n * blocks + b];
    mse[n] = s / count;
  }
}

bool bad_image(int N, int H, int W, int C) {
  return N < 1 || H < 1 || W < 1 || C < 1 || N > 65535 || (double)H * W * C > 2147483647.0;
}

// a [H, cols] region with row stride ld inside an image of stride `image`: rows may not overlap, nor may images
bool bad_strides(long ld, long image, int N, int H, long cols) {
  return ld < cols || (N > 1 && image < (long)(H - 1) * ld + cols);
}

bool misaligned(const void* ptr, unsigned a) { return ((uintptr_t)ptr & (a - 1)) != 0; }

long cc_bytes(int N, int H, int W, int K, long* off_warps, long* off_sse, long* off_flags) {
  const long B = grid_blocks((long)H * W, THREADS, MAX_BLOCKS);
  const long part = (long)N * 3 * B * NS, warps = (long)N * K * 3 * NF, sse = (long)N * B, flags = (long)N * K * 3;
  if (off_warps) *off_warps = part;
  if (off_sse) *off_sse = part + warps;
  if (off_flags) *off_flags = part + warps + sse;
  return (part + warps + sse) * (long)sizeof(double) + ((flags + 1) / 2 * 2) * (long)sizeof(int);
}

}  // namespace

extern "C" long v3a_color_correct_workspace_bytes(int N, int H, int W, int num_iters) {
  if (bad_image(N, H, W, 3) || num_iters < 1 || num_iters > MAX_ITERS) return V3A_ERR_SHAPE;
  return cc_bytes(N, H, W, num_iters, nullptr, nullptr, nullptr);
}

extern "C" int v3a_color_correct(const v3a_color_correct_args* a, void* stream) {
  if (!a || !a->img || !a->ref || !a->out || !a->sse || !a->status) return V3A_ERR_ARG;
  if (misaligned(a->img, 4) || misaligned(a->ref, 4) || misaligned(a->out, 4) || misaligned(a->sse, 8) || misaligned(a->status, 4))
    return V3A_ERR_ARG;
  if (bad_image(a->N, a->H, a->W, 3) || a->num_iters < 1 || a->num_iters > MAX_ITERS) return V3A_ERR_SHAPE;
  const long cols = 3L * a->W;
  if (bad_strides(a->ld_img, a->img_stride, a->N, a->H, cols) || bad_strides(a->ld_ref, a->ref_stride, a->N, a->H, cols) ||
      bad_strides(a->ld_out, a->out_stride, a->N, a->H, cols))
    return V3A_ERR_SHAPE;
  if (!(a->eps >= 0.0 && a->eps < 0.5)) return V3A_ERR_ARG;
  long off_warps, off_sse, off_flags;
  const long need = cc_bytes(a->N, a->H, a->W, a->num_iters, &off_warps, &off_sse, &off_flags);
  if (!a->workspace || misaligned(a->workspace, 8) || a->workspace_bytes < need) return V3A_ERR_WORKSPACE;

  CcP p;
  p.img = a->img; p.ref = a->ref; p.out = a->out;
  p.ld_img = a->ld_img; p.ld_ref = a->ld_ref; p.ld_out = a->ld_out;
  p.img_stride = a->img_stride; p.ref_stride = a->ref_stride; p.out_stride = a->out_stride;
  p.N = a->N; p.H = a->H; p.W = a->W; p.K = a->num_iters;
  p.lo = a->eps; p.hi = 1.0 - a->eps;
  double* ws = (double*)a->workspace;
  p.part = ws;
  p.warps = ws + off_warps;
  p.part_sse = ws + off_sse;
  p.flags = (int*)(ws + off_flags);
  const int B = grid_blocks((long)p.H * p.W, THREADS, MAX_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  for (int it = 0; it < p.K; ++it) {
    hipLaunchKernelGGL(cc_accumulate_kernel, dim3(B, 3, p.N), dim3(THREADS), 0, st, p, it);
    if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
    hipLaunchKernelGGL(cc_solve_kernel, dim3(3, p.N), dim3(SOLVE_THREADS), 0, st, p, it, B);
    if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(cc_apply_kernel, dim3(B, p.N), dim3(THREADS), 0, st, p);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(cc_finish_kernel, dim3(p.N), dim3(64), 0, st, p, B, a->sse, a->status);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" long v3a_image_mse_workspace_bytes(int N, int H, int W, int C) {
  if (bad_image(N, H, W, C)) return V3A_ERR_SHAPE;
  return (long)N * grid_blocks((long)H * W * C, THREADS, MAX_BLOCKS) * (long)sizeof(double);
}

extern "C" int v3a_image_mse(const v3a_image_mse_args* a, void* stream) {
  if (!a || !a->a || !a->b || !a->mse) return V3A_ERR_ARG;
  if (misaligned(a->a, 4) || misaligned(a->b, 4) || misaligned(a->mse, 8)) return V3A_ERR_ARG;
  if (bad_image(a->N, a->H, a->W, a->C)) return V3A_ERR_SHAPE;
  const long cols = (long)a->W * a->C;
  if (bad_strides(a->ld_a, a->a_stride, a->N, a->H, cols) || bad_strides(a->ld_b, a->b_stride, a->N, a->H, cols)) return V3A_ERR_SHAPE;
  const long need = v3a_image_mse_workspace_bytes(a->N, a->H, a->W, a->C);
  if (!a->workspace || misaligned(a->workspace, 8) || a->workspace_bytes < need) return V3A_ERR_WORKSPACE;
  MseP p;
  p.a = a->a; p.b = a->b;
  p.ld_a = a->ld_a; p.ld_b = a->ld_b; p.a_stride = a->a_stride; p.b_stride = a->b_stride;
  p.N = a->N; p.H = a->H; p.W = a->W; p.C = a->C;
  const int B = grid_blocks((long)p.H * p.W * p.C, THREADS, MAX_BLOCKS);
  double* part = (double*)a->workspace;
  hipLaunchKernelGGL(mse_partial_kernel, dim3(B, p.N), dim3(THREADS), 0, (hipStream_t)stream, p, part);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(mse_finish_kernel, dim3(p.N), dim3(64), 0, (hipStream_t)stream, part, B, (double)p.H * p.W * p.C, a->mse);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
