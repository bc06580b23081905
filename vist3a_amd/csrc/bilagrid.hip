// Bilateral-grid colour compensation of the post-optimisation loop: slice + affine apply (forward, backward) and the total-variation
// regulariser (forward, backward).  third_party_model/anysplat/src/post_opt/lib_bilagrid.py::BilateralGrid / slice /
// total_variation_loss, the 5-D case (one grid per image).
//
// Layout: rgb f32 [N,H,W,3] (the rasteriser's), grids f32 [N,L,GY,GX,12] coefficient-minor: a vertex's 12 coefficients are three
// 16-byte loads; coefficient 4c + k is row c, column k of the 3x4 matrix (the reference's reshape(..., 3, 4) of its channel axis).
// GX, GY, L >= 2 (smaller: V3A_ERR_SHAPE; the reference degenerates silently).
//
// Slice, per pixel (i, j), fp64 after the loads:
//   x = (j + 0.5) / W, y = (i + 0.5) / H           computed here: there is no grid_xy tensor
//   gray = 0.299f r + 0.587f g + 0.114f b           the float32 weights widened, as the reference's float32 buffer holds them
//   ix = x (GX-1), iy = y (GY-1), iz = clamp(gray (L-1), 0, L-1)        grid_sample(bilinear, align_corners=True, border)
//   lower corner by floor; an upper corner past the end has weight 0 and is not read
//   A = trilinear blend of the 8 vertices' coefficients;  out[c] = A[c][0] r + A[c][1] g + A[c][2] b + A[c][3], rounded once
// Backward, d_rgb (one thread per pixel, as the forward):
//   d_rgb[k] = sum_c A[c][k] d_out[c] + w_k (L-1) dL/diz,  dL/diz = sum_{c,k} d_out[c] [r,g,b,1][k] (P1 - P0)[c][k]
//   with P0, P1 the x-y-bilinear blends of the lower and upper plane; the guidance term is exactly 0 where gray (L-1) <= 0 or
//   >= L-1 (torch's clip_coordinates_set_grad); on an interior plane floor() gives the right derivative.
// Backward, d_grids: a gather, no atomics, nothing memset.  One workgroup per VERTEX (n, l, gy, gx), 256 threads over the pixels of
// its x-y support (|ix - gx| < 1, |iy - gy| < 1: a window computed with a pixel of margin, the weight itself decides), each thread
// 12 fp64 accumulators (d_out[c] [r,g,b,1][k] times the vertex's trilinear weight, 0 for a pixel whose iz is a plane away), then one
// fixed-order LDS tree over the threads: every element written exactly once, zeros included, bit-identical run to run, and exactly
// linear in d_out.  A pixel is visited by 4 L workgroups (its four columns, every plane); at 448^2 on 16 x 16 x 8 that is 6.4e6
// visits of a few dozen flops against L2-resident rgb / d_out.  The form with one workgroup per (gy, gx) column and threads laid out
// as slices x 12 L outputs does the same redundant weight arithmetic and ties the workgroup's shape to L; this one has no limit
// on L and 2048 workgroups at the default shape for the 256 CUs.
// The forward reads its 8 vertices from global memory (the default grid is 98 KB per view: L2-resident); staging the vertex columns
// of a pixel tile in LDS is not done and whether it would pay is not measured.
//
// Total variation of [V,L,GY,GX,12]: for each of the axes L, GY, GX the sum of squared forward differences divided by
// 12 * (L GY GX with that axis' size - 1), added in that order and divided by V.  fp64 partials per workgroup (one per axis) on a grid
// that depends on the size only, then a one-workgroup reduction (fixed_sum.h).  Backward: one launch, every element written once,
// d_out times a coefficient that does not depend on it.
#include "common.h"
#include "fixed_sum.h"
#include "../../include/vist3a_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 2048;

struct SliceP {
  const float* rgb; const float* grids;
  int N, H, W, GX, GY, L;
  int vec;                            // grids is 16-byte aligned: a vertex is three 16-byte loads
};

struct Axis { int i0; double t; };    // lower corner and the weight of the upper one

__device__ __forceinline__ Axis axis_at(double f, int size) {
  f = fmin(fmax(f, 0.0), (double)(size - 1));
  const double fl = floor(f);
  Axis a;
  a.i0 = (int)fl;
  a.t = f - fl;
  return a;
}

__device__ __forceinline__ Axis axis_xy(int idx, int n_px, int size) {
  return axis_at((((double)idx + 0.5) / (double)n_px) * (double)(size - 1), size);
}

// live: the guidance coordinate is strictly inside (0, L-1), where it has a gradient
__device__ __forceinline__ Axis axis_z(float r, float g, float b, int L, bool& live) {
  const double gray = (double)0.299f * (double)r + (double)0.587f * (double)g + (double)0.114f * (double)b;
  const double f = gray * (double)(L - 1);
  live = f > 0.0 && f < (double)(L - 1);
  return axis_at(f, L);
}

__device__ __forceinline__ void load12(const float* g, int vec, float (&v)[12]) {
  if (vec) {
    const float4 a = ((const float4*)g)[0], b = ((const float4*)g)[1], c = ((const float4*)g)[2];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
  } else {
#pragma unroll
    for (int q = 0; q < 12; ++q) v[q] = g[q];
  }
}

// x-y-bilinear blend of one plane (base = the plane's first vertex)
__device__ __forceinline__ void plane_blend(const SliceP& p, const float* base, Axis ax, Axis ay, double (&P)[12]) {
#pragma unroll
  for (int q = 0; q < 12; ++q) P[q] = 0.0;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
    const int yy = ay.i0 + dy;
    if (yy > p.GY - 1) continue;
    const double wy = dy ? ay.t : 1.0 - ay.t;
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int xx = ax.i0 + dx;
      if (xx > p.GX - 1) continue;
      const double w = (dx ? ax.t : 1.0 - ax.t) * wy;
      float v[12];
      load12(base + ((long)yy * p.GX + xx) * 12, p.vec, v);
#pragma unroll
      for (int q = 0; q < 12; ++q) P[q] += w * (double)v[q];
    }
  }
}

// P0, P1: the blends of the planes az.i0 and az.i0 + 1 (zeros where that plane is past the end) for pixel `px` of the flat [N,H,W]
__device__ __forceinline__ void pixel_planes(const SliceP& p, long px, float r, float g, float b, Axis& az, bool& live,
                                             double (&P0)[12], double (&P1)[12]) {
  const int j = (int)(px % p.W), i = (int)((px / p.W) % p.H), n = (int)(px / ((long)p.W * p.H));
  const Axis ax = axis_xy(j, p.W, p.GX), ay = axis_xy(i, p.H, p.GY);
  az = axis_z(r, g, b, p.L, live);
  const long plane = (long)p.GY * p.GX * 12;
  const float* base = p.grids + ((long)n * p.L + az.i0) * plane;
  plane_blend(p, base, ax, ay, P0);
  if (az.i0 + 1 <= p.L - 1) {
    plane_blend(p, base + plane, ax, ay, P1);
  } else {
#pragma unroll
    for (int q = 0; q < 12; ++q) P1[q] = 0.0;
  }
}

__global__ void __launch_bounds__(THREADS) bilagrid_slice_fwd_kernel(const SliceP p, float* out) {
  const long n_px = (long)p.N * p.H * p.W;
  const long stride = (long)gridDim.x * THREADS;
  for (long px = (long)blockIdx.x * THREADS + threadIdx.x; px < n_px; px += stride) {
    const float r = p.rgb[px * 3], g = p.rgb[px * 3 + 1], b = p.rgb[px * 3 + 2];
    Axis az;
    bool live;
    double P0[12], P1[12];
    pixel_planes(p, px, r, g, b, az, live, P0, P1);
    const double w0 = 1.0 - az.t, w1 = az.t;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double A[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) A[k] = w0 * P0[4 * c + k] + w1 * P1[4 * c + k];
      out[px * 3 + c] = (float)(A[0] * (double)r + A[1] * (double)g + A[2] * (double)b + A[3]);
    }
  }
}

__global__ void __launch_bounds__(THREADS) bilagrid_slice_bwd_rgb_kernel(const SliceP p, const float* d_out, float* d_rgb) {
  const long n_px = (long)p.N * p.H * p.W;
  const long stride = (long)gridDim.x * THREADS;
  for (long px = (long)blockIdx.x * THREADS + threadIdx.x; px < n_px; px += stride) {
    const float r = p.rgb[px * 3], g = p.rgb[px * 3 + 1], b = p.rgb[px * 3 + 2];
    const double go[3] = {(double)d_out[px * 3], (double)d_out[px * 3 + 1], (double)d_out[px * 3 + 2]};
    const double in[4] = {(double)r, (double)g, (double)b, 1.0};
    Axis az;
    bool live;
    double P0[12], P1[12];
    pixel_planes(p, px, r, g, b, az, live, P0, P1);
    const double w0 = 1.0 - az.t, w1 = az.t;
    double d[3] = {0.0, 0.0, 0.0}, diz = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double a = w0 * P0[4 * c + k] + w1 * P1[4 * c + k];
        if (k < 3) d[k] += a * go[c];
        diz += (go[c] * in[k]) * (P1[4 * c + k] - P0[4 * c + k]);
      }
    }
    if (live) {
      const double s = (double)(p.L - 1) * diz;
      d[0] += (double)0.299f * s;
      d[1] += (double)0.587f * s;
      d[2] += (double)0.114f * s;
    }
    d_rgb[px * 3] = (float)d[0];
    d_rgb[px * 3 + 1] = (float)d[1];
    d_rgb[px * 3 + 2] = (float)d[2];
  }
}

// the weight of vertex `v` of an axis for a sample whose lower corner is a.i0
__device__ __forceinline__ double vertex_weight(Axis a, int v) {
  return a.i0 == v ? 1.0 - a.t : (a.i0 + 1 == v ? a.t : 0.0);
}

// first and last pixel (inclusive, clamped) that can have |pos (size-1) - v| < 1, one pixel of margin on either side
__device__ __forceinline__ void support(int v, int size, int n_px, int& lo, int& hi) {
  const double s = (double)n_px / (double)(size - 1);
  const double a = floor((double)(v - 1) * s - 0.5) - 1.0, b = ceil((double)(v + 1) * s - 0.5) + 1.0;
  lo = (int)fmax(a, 0.0);
  hi = (int)fmin(b, (double)(n_px - 1));
}

// one workgroup per vertex, blockIdx.x = ((n L + l) GY + gy) GX + gx = the vertex's index in d_grids
__global__ void __launch_bounds__(THREADS) bilagrid_slice_bwd_grid_kernel(const SliceP p, const float* d_out, float* d_grids) {
  __shared__ double red[12][THREADS];
  const int t = threadIdx.x;
  const long v = blockIdx.x;
  const int gx = (int)(v % p.GX), gy = (int)((v / p.GX) % p.GY), l = (int)((v / ((long)p.GX * p.GY)) % p.L);
  const int n = (int)(v / ((long)p.GX * p.GY * p.L));
  int x_lo, x_hi, y_lo, y_hi;
  support(gx, p.GX, p.W, x_lo, x_hi);
  support(gy, p.GY, p.H, y_lo, y_hi);
  const int wpx = x_hi - x_lo + 1, hpx = y_hi - y_lo + 1;
  double acc[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) acc[q] = 0.0;
  for (int s = t; s < wpx * hpx; s += THREADS) {
    const int i = y_lo + s / wpx, j = x_lo + s % wpx;
    const double wxy = vertex_weight(axis_xy(j, p.W, p.GX), gx) * vertex_weight(axis_xy(i, p.H, p.GY), gy);
    if (wxy == 0.0) continue;
    const long px = ((long)n * p.H + i) * p.W + j;
    const float r = p.rgb[px * 3], g = p.rgb[px * 3 + 1], b = p.rgb[px * 3 + 2];
    bool live;
    const double w = wxy * vertex_weight(axis_z(r, g, b, p.L, live), l);
    if (w == 0.0) continue;
    const double in[4] = {(double)r, (double)g, (double)b, 1.0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double wg = w * (double)d_out[px * 3 + c];
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[4 * c + k] += wg * in[k];
    }
  }
#pragma unroll
  for (int q = 0; q < 12; ++q) red[q][t] = acc[q];
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int q = 0; q < 12; ++q) red[q][t] += red[q][t + s];
    }
    __syncthreads();
  }
  if (t < 12) d_grids[v * 12 + t] = (float)red[t][0];
}

// ---------------------------------------------------------------------------------------------------- total variation
struct TvP {
  const float* grids;
  int V, GX, GY, L;
  long n;                             // V L GY GX 12
};

// part[0..2][blocks]: squared forward differences along L, GY, GX
__global__ void __launch_bounds__(THREADS) bilagrid_tv_fwd_kernel(const TvP p, double* part) {
  __shared__ double red[THREADS];
  const long sx = 12, sy = 12L * p.GX, sl = 12L * p.GX * p.GY;
  const long stride = (long)gridDim.x * THREADS;
  double al = 0.0, ay = 0.0, ax = 0.0;
  for (long e = (long)blockIdx.x * THREADS + threadIdx.x; e < p.n; e += stride) {
    const int x = (int)((e / sx) % p.GX), y = (int)((e / sy) % p.GY), l = (int)((e / sl) % p.L);
    const double c = (double)p.grids[e];
    if (l < p.L - 1) { const double d = (double)p.grids[e + sl] - c; al += d * d; }
    if (y < p.GY - 1) { const double d = (double)p.grids[e + sy] - c; ay += d * d; }
    if (x < p.GX - 1) { const double d = (double)p.grids[e + sx] - c; ax += d * d; }
  }
  const double tl = block_sum<THREADS>(al, red), ty = block_sum<THREADS>(ay, red), tx = block_sum<THREADS>(ax, red);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = tl;
    part[gridDim.x + blockIdx.x] = ty;
    part[2 * gridDim.x + blockIdx.x] = tx;
  }
}

__device__ __forceinline__ double count_l(const TvP& p) { return 12.0 * (double)(p.L - 1) * (double)p.GY * (double)p.GX; }
__device__ __forceinline__ double count_y(const TvP& p) { return 12.0 * (double)p.L * (double)(p.GY - 1) * (double)p.GX; }
__device__ __forceinline__ double count_x(const TvP& p) { return 12.0 * (double)p.L * (double)p.GY * (double)(p.GX - 1); }

__global__ void __launch_bounds__(THREADS) bilagrid_tv_reduce_kernel(const TvP p, const double* part, int parts, double* out) {
  __shared__ double red[THREADS];
  double s[3];
  for (int a = 0; a < 3; ++a) {
    double v = 0.0;
    for (int t = threadIdx.x; t < parts; t += THREADS) v += part[(long)a * parts + t];
    s[a] = block_sum<THREADS>(v, red);
  }
  if (threadIdx.x == 0) out[0] = (s[0] / count_l(p) + s[1] / count_y(p) + s[2] / count_x(p)) / (double)p.V;
}

__global__ void __launch_bounds__(THREADS) bilagrid_tv_bwd_kernel(const TvP p, const double* d_out, float* d_grids) {
  const long sx = 12, sy = 12L * p.GX, sl = 12L * p.GX * p.GY;
  const long stride = (long)gridDim.x * THREADS;
  const double g = d_out[0];
  const double cl = count_l(p), cy = count_y(p), cx = count_x(p);
  for (long e = (long)blockIdx.x * THREADS + threadIdx.x; e < p.n; e += stride) {
    const int x = (int)((e / sx) % p.GX), y = (int)((e / sy) % p.GY), l = (int)((e / sl) % p.L);
    const double c = (double)p.grids[e];
    double dl = 0.0, dy = 0.0, dx = 0.0;
    if (l > 0) dl += c - (double)p.grids[e - sl];
    if (l < p.L - 1) dl -= (double)p.grids[e + sl] - c;
    if (y > 0) dy += c - (double)p.grids[e - sy];
    if (y < p.GY - 1) dy -= (double)p.grids[e + sy] - c;
    if (x > 0) dx += c - (double)p.grids[e - sx];
    if (x < p.GX - 1) dx -= (double)p.grids[e + sx] - c;
    d_grids[e] = (float)(g * (2.0 * (dl / cl + dy / cy + dx / cx) / (double)p.V));
  }
}

bool bad_grid(int V, int GX, int GY, int L) {
  return V < 1 || GX < 2 || GY < 2 || L < 2 || (double)V * GX * GY * L * 12.0 > 2147483647.0;
}

bool bad_slice(const v3a_bilagrid_slice_args* a) {
  return a->N < 1 || a->H < 1 || a->W < 1 || (double)a->N * a->H * a->W * 3.0 > 2147483647.0 || bad_grid(a->N, a->GX, a->GY, a->L);
}

SliceP slice_params(const v3a_bilagrid_slice_args* a) {
  SliceP p;
  p.rgb = a->rgb; p.grids = a->grids;
  p.N = a->N; p.H = a->H; p.W = a->W; p.GX = a->GX; p.GY = a->GY; p.L = a->L;
  p.vec = ((uintptr_t)a->grids & 15) ? 0 : 1;
  return p;
}

TvP tv_params(const v3a_bilagrid_tv_args* a) {
  TvP p;
  p.grids = a->grids;
  p.V = a->V; p.GX = a->GX; p.GY = a->GY; p.L = a->L;
  p.n = (long)a->V * a->L * a->GY * a->GX * 12;
  return p;
}

}  // namespace

extern "C" int v3a_bilagrid_slice_forward(const v3a_bilagrid_slice_args* a, float* out, void* stream) {
  if (!a || !a->rgb || !a->grids || !out) return V3A_ERR_ARG;
  if (bad_slice(a)) return V3A_ERR_SHAPE;
  const SliceP p = slice_params(a);
  hipLaunchKernelGGL(bilagrid_slice_fwd_kernel, dim3(grid_blocks((long)p.N * p.H * p.W, THREADS, MAX_BLOCKS)), dim3(THREADS), 0, (hipStream_t)stream, p, out);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_bilagrid_slice_backward(const v3a_bilagrid_slice_args* a, const float* d_out, float* d_rgb, float* d_grids, void* stream) {
  if (!a || !a->rgb || !a->grids || !d_out || (!d_rgb && !d_grids)) return V3A_ERR_ARG;
  if (bad_slice(a)) return V3A_ERR_SHAPE;
  const SliceP p = slice_params(a);
  if (d_rgb) {
    hipLaunchKernelGGL(bilagrid_slice_bwd_rgb_kernel, dim3(grid_blocks((long)p.N * p.H * p.W, THREADS, MAX_BLOCKS)), dim3(THREADS), 0, (hipStream_t)stream, p, d_out, d_rgb);
    if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  }
  if (d_grids) {
    const long vertices = (long)p.N * p.L * p.GY * p.GX;
    hipLaunchKernelGGL(bilagrid_slice_bwd_grid_kernel, dim3((unsigned)vertices), dim3(THREADS), 0, (hipStream_t)stream, p, d_out, d_grids);
    if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  }
  return V3A_OK;
}

extern "C" long v3a_bilagrid_tv_workspace_bytes(int V, int GX, int GY, int L) {
  if (bad_grid(V, GX, GY, L)) return V3A_ERR_SHAPE;
  return 3L * grid_blocks((long)V * L * GY * GX * 12, THREADS, MAX_BLOCKS) * (long)sizeof(double);
}

extern "C" int v3a_bilagrid_tv_forward(const v3a_bilagrid_tv_args* a, void* stream) {
  if (!a || !a->grids || !a->out) return V3A_ERR_ARG;
  if (bad_grid(a->V, a->GX, a->GY, a->L)) return V3A_ERR_SHAPE;
  if (!a->workspace || ((uintptr_t)a->workspace & 7) || a->workspace_bytes < v3a_bilagrid_tv_workspace_bytes(a->V, a->GX, a->GY, a->L))
    return V3A_ERR_WORKSPACE;
  const TvP p = tv_params(a);
  const int blocks = grid_blocks(p.n, THREADS, MAX_BLOCKS);
  double* part = (double*)a->workspace;
  hipLaunchKernelGGL(bilagrid_tv_fwd_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, p, part);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(bilagrid_tv_reduce_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, p, part, blocks, a->out);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_bilagrid_tv_backward(const v3a_bilagrid_tv_args* a, const double* d_out, float* d_grids, void* stream) {
  if (!a || !a->grids || !d_out || !d_grids) return V3A_ERR_ARG;
  if (bad_grid(a->V, a->GX, a->GY, a->L)) return V3A_ERR_SHAPE;
  const TvP p = tv_params(a);
  hipLaunchKernelGGL(bilagrid_tv_bwd_kernel, dim3(grid_blocks(p.n, THREADS, MAX_BLOCKS)), dim3(THREADS), 0, (hipStream_t)stream, p, d_out, d_grids);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
