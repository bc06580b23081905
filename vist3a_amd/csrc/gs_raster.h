// The forward math of the 3D-Gaussian rasteriser, written once: the forward (raster.hip) computes it, the backward (raster_bwd.hip)
// recomputes it and has to land on the same values, bit for bit.  SH basis and colour, the projection chain of one (camera,
// Gaussian) entry, the tile rectangle and its count + scan, LDS staging, the alpha of a pixel-Gaussian pair, the front-to-back walk
// of a tile list, and the host-side checks of the entry points.  The pure math is __host__ __device__: a CPU build stays possible.
#pragma once
#include <rocprim/device/device_scan.hpp>
#include <type_traits>

#include "common.h"
#include "../../include/vist3a_hip.h"

namespace gs {

constexpr int TILE = 16;

template <int DEG>
__host__ __device__ __forceinline__ void sh_eval(float x, float y, float z, float* b) {
  b[0] = 0.2820947917738781f;
  if constexpr (DEG >= 1) { b[1] = -0.48860251190292f * y; b[2] = 0.48860251190292f * z; b[3] = -0.48860251190292f * x; }
  if constexpr (DEG >= 2) {
    const float z2 = z * z, t0b = -1.092548430592079f * z, c1 = x * x - y * y, s1 = 2.f * x * y;
    const float p6 = 0.9461746957575601f * z2 - 0.3153915652525201f;
    b[4] = 0.5462742152960395f * s1; b[5] = t0b * y; b[6] = p6; b[7] = t0b * x; b[8] = 0.5462742152960395f * c1;
    if constexpr (DEG >= 3) {
      const float t0c = -2.285228997322329f * z2 + 0.4570457994644658f, t1b = 1.445305721320277f * z;
      const float c2 = x * c1 - y * s1, s2 = x * s1 + y * c1;
      const float p12 = z * (1.865881662950577f * z2 - 1.119528997770346f);
      b[9] = -0.5900435899266435f * s2; b[10] = t1b * s1; b[11] = t0c * y; b[12] = p12; b[13] = t0c * x; b[14] = t1b * c1;
      b[15] = -0.5900435899266435f * c2;
      if constexpr (DEG >= 4) {
        const float t0d = z * (-4.683325804901025f * z2 + 2.007139630671868f), t1c = 3.31161143515146f * z2 - 0.47308734787878f;
        const float t2b = -1.770130769779931f * z, c3 = x * c2 - y * s2, s3 = x * s2 + y * c2;
        b[16] = 0.6258357354491763f * s3; b[17] = t2b * s2; b[18] = t1c * s1; b[19] = t0d * y;
        b[20] = 1.984313483298443f * z * p12 - 1.006230589874905f * p6;
        b[21] = t0d * x; b[22] = t1c * c1; b[23] = t2b * c2; b[24] = 0.6258357354491763f * c3;
      }
    }
  }
}

// SH colour of one Gaussian before the +0.5 / clamp: s = its SH row, [K, 3] (sh_layout 0) or [3, K] (1)
template <int DEG>
__host__ __device__ __forceinline__ void sh_color(const float* bas, const float* s, int sh_layout, int sh_k, float& r, float& g, float& b) {
  constexpr int NB = (DEG + 1) * (DEG + 1);
  r = g = b = 0.f;
  if (sh_layout == 0) {  // [U, K, 3]
#pragma unroll
    for (int k = 0; k < NB; ++k) { r += bas[k] * s[3 * k]; g += bas[k] * s[3 * k + 1]; b += bas[k] * s[3 * k + 2]; }
  } else {  // [U, 3, K]
#pragma unroll
    for (int k = 0; k < NB; ++k) { r += bas[k] * s[k]; g += bas[k] * s[sh_k + k]; b += bas[k] * s[2 * sh_k + k]; }
  }
}

// One wave stages `total` floats (the SH rows of its 64 Gaussians) into LDS: 16-byte loads where the source is aligned
__device__ __forceinline__ void stage_sh_rows(float* s_sh, const float* src, int total, int lane) {
  if ((((unsigned long long)(uintptr_t)src) & 15) == 0) {
    const int n4 = total >> 2;
    for (int i = lane; i < n4; i += 64) *(f32x4*)(s_sh + 4 * i) = *(const f32x4*)(src + 4 * i);
    for (int i = (n4 << 2) + lane; i < total; i += 64) s_sh[i] = src[i];
  } else {
    for (int i = lane; i < total; i += 64) s_sh[i] = src[i];
  }
}

// ---------------------------------------------------------------------------------------------- projection of one entry
struct ProjEntry {
  float x, y, z, rz, rz2;                 // camera-space mean, 1 / z, 1 / z^2
  float fx, fy, cx, cy;                   // intrinsics
  float lxp, lxn, lyp, lyn;               // clamp limits of x / z and y / z
  float tx, ty, j00, j02, j11, j12;       // clamped mean, J = [[j00, 0, j02], [0, j11, j12]]
  float c00, c01, c02, c11, c12, c22;     // Cc = R S R^T (symmetric)
  float t00, t01, t02, t10, t11, t12;     // J Cc (t10: the backward's; dead in the forward)
  float q00, q01, q11, det;               // cov2d = J Cc J^T + eps2d, its determinant
  float det_orig;                         // determinant of J Cc J^T itself: project_entry<true> only (antialiased mode), else 0
};

// world -> camera: V = view matrix (4x4 row-major), (mx, my, mz) = world mean
__host__ __device__ __forceinline__ void to_camera(const float* V, float mx, float my, float mz, float& x, float& y, float& z) {
  const float R00 = V[0], R01 = V[1], R02 = V[2], R10 = V[4], R11 = V[5], R12 = V[6], R20 = V[8], R21 = V[9], R22 = V[10];
  x = R00 * mx + R01 * my + R02 * mz + V[3];
  y = R10 * mx + R11 * my + R12 * mz + V[7];
  z = R20 * mx + R21 * my + R22 * mz + V[11];
}

// Kc = intrinsics (3x3), (x, y, z) = to_camera's mean, s.. = upper triangle of the world covariance.  No test is made here: near /
// far (on z, before) and det > 0 (after) are the caller's.  AA adds det_orig.  It is a template argument, and the classic callers
// instantiate <false>, because lines that merely stand in the function - dead ones included - change how hipcc packs and contracts
// the expressions of q00 / q01 / q11 / det (seen in the ISA), and with that the last bits of every classic output.
template <bool AA = false>
__host__ __device__ __forceinline__ ProjEntry project_entry(const float* V, const float* Kc, float W, float H, float eps2d, float x,
                                                            float y, float z, float s00, float s01, float s02, float s11, float s12,
                                                            float s22) {
  const float R00 = V[0], R01 = V[1], R02 = V[2], R10 = V[4], R11 = V[5], R12 = V[6], R20 = V[8], R21 = V[9], R22 = V[10];
  // M = R * S
  const float a00 = R00 * s00 + R01 * s01 + R02 * s02, a01 = R00 * s01 + R01 * s11 + R02 * s12, a02 = R00 * s02 + R01 * s12 + R02 * s22;
  const float a10 = R10 * s00 + R11 * s01 + R12 * s02, a11 = R10 * s01 + R11 * s11 + R12 * s12, a12 = R10 * s02 + R11 * s12 + R12 * s22;
  const float a20 = R20 * s00 + R21 * s01 + R22 * s02, a21 = R20 * s01 + R21 * s11 + R22 * s12, a22 = R20 * s02 + R21 * s12 + R22 * s22;
  // Cc = M * R^T (symmetric)
  const float c00 = a00 * R00 + a01 * R01 + a02 * R02, c01 = a00 * R10 + a01 * R11 + a02 * R12, c02 = a00 * R20 + a01 * R21 + a02 * R22;
  const float c11 = a10 * R10 + a11 * R11 + a12 * R12, c12 = a10 * R20 + a11 * R21 + a12 * R22;
  const float c22 = a20 * R20 + a21 * R21 + a22 * R22;
  const float fx = Kc[0], fy = Kc[4], cx = Kc[2], cy = Kc[5];
  const float tfx = 0.5f * W / fx, tfy = 0.5f * H / fy;
  const float lxp = (W - cx) / fx + 0.3f * tfx, lxn = cx / fx + 0.3f * tfx;
  const float lyp = (H - cy) / fy + 0.3f * tfy, lyn = cy / fy + 0.3f * tfy;
  const float rz = 1.f / z, rz2 = rz * rz;
  const float tx = z * fminf(lxp, fmaxf(-lxn, x * rz)), ty = z * fminf(lyp, fmaxf(-lyn, y * rz));
  const float j00 = fx * rz, j02 = -fx * tx * rz2, j11 = fy * rz, j12 = -fy * ty * rz2;
  // cov2d = J Cc J^T, J = [[j00,0,j02],[0,j11,j12]]
  const float t00 = j00 * c00 + j02 * c02, t01 = j00 * c01 + j02 * c12, t02 = j00 * c02 + j02 * c22;
  const float t10 = j11 * c01 + j12 * c02, t11 = j11 * c11 + j12 * c12, t12 = j11 * c12 + j12 * c22;
  const float q00 = t00 * j00 + t02 * j02 + eps2d;
  const float q01 = t01 * j11 + t02 * j12;
  const float q11 = t11 * j11 + t12 * j12 + eps2d;
  const float det = q00 * q11 - q01 * q01;
  float det_orig = 0.f;
  if constexpr (AA) {  // the un-blurred J Cc J^T from expressions of its own: q00 / q01 / q11 above stay as they are written
    const float o00 = t00 * j00 + t02 * j02, o01 = t01 * j11 + t02 * j12, o11 = t11 * j11 + t12 * j12;
    det_orig = o00 * o11 - o01 * o01;
  }
  return {x, y, z, rz, rz2, fx, fy, cx, cy, lxp, lxn, lyp, lyn, tx, ty, j00, j02, j11, j12, c00, c01, c02, c11, c12, c22,
          t00, t01, t02, t10, t11, t12, q00, q01, q11, det, det_orig};
}

// Antialiased mode (gsplat rasterize_mode="antialiased", the Mip-Splatting 2D filter): the blur widens a Gaussian AND dims it by
// comp = sqrt(det(J Cc J^T) / det(J Cc J^T + eps2d I)), r = comp^2.  e from project_entry<true>, valid where e.det > 0.
__host__ __device__ __forceinline__ float compensation(const ProjEntry& e, float& r) {
  r = fmaxf(0.f, e.det_orig / e.det);
  return sqrtf(r);
}

// ---------------------------------------------------------------------------------------------- tiles
struct TileGrid { int tw, th, ntiles; };
inline TileGrid tile_grid(int width, int height) {
  const int tw = (width + TILE - 1) / TILE, th = (height + TILE - 1) / TILE;
  return {tw, th, tw * th};
}

__host__ __device__ __forceinline__ void tile_bounds(float mx, float my, int radius, int tw, int th, int& x0, int& x1, int& y0, int& y1) {
  const float r = (float)radius / (float)TILE, tx = mx / (float)TILE, ty = my / (float)TILE;
  // (uint32)floor(negative) saturates to 0 on the device gsplat runs on: clamp to [0, grid]
  x0 = (int)fminf(fmaxf(floorf(tx - r), 0.f), (float)tw); x1 = (int)fminf(fmaxf(ceilf(tx + r), 0.f), (float)tw);
  y0 = (int)fminf(fmaxf(floorf(ty - r), 0.f), (float)th); y1 = (int)fminf(fmaxf(ceilf(ty + r), 0.f), (float)th);
}

// tiles that camera-Gaussian entry e touches (0 for a culled one)
__host__ __device__ __forceinline__ unsigned int entry_tile_count(const int* radii, const float* means2d, long e, int tw, int th) {
  const int r = radii[e];
  if (r <= 0) return 0;
  int x0, x1, y0, y1;
  tile_bounds(means2d[2 * e], means2d[2 * e + 1], r, tw, th, x0, x1, y0, y1);
  return (unsigned int)((x1 - x0) * (y1 - y0));
}

struct CountP { const int* radii; const float* means2d; long CU; int tw, th; unsigned int* counts; };  // CU = C * U entries

static __global__ __launch_bounds__(256) void gs_count_kernel(CountP p) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < p.CU) p.counts[e] = entry_tile_count(p.radii, p.means2d, e, p.tw, p.th);
}


inline size_t scan_tmp_bytes(long CU) {
  size_t t = 0;
  (void)rocprim::inclusive_scan(nullptr, t, (unsigned int*)nullptr, (unsigned int*)nullptr, (size_t)CU, rocprim::plus<unsigned int>());
  return t;
}

// counts[e] = tiles of entry e, incl = their inclusive scan (entry e's intersections / row slots start at incl[e] - counts[e])
inline bool count_and_scan(const CountP& p, unsigned int* incl, void* tmp, size_t tmp_bytes, hipStream_t stream) {
  hipLaunchKernelGGL(gs_count_kernel, dim3((unsigned)((p.CU + 255) / 256)), dim3(256), 0, stream, p);
  return rocprim::inclusive_scan(tmp, tmp_bytes, p.counts, incl, (size_t)p.CU, rocprim::plus<unsigned int>(), stream) == hipSuccess;
}

// ---------------------------------------------------------------------------------------------- compositing
__host__ __device__ __forceinline__ float fast_exp(float x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __expf(x);
#else
  return expf(x);
#endif
}

// Stage one Gaussian of a tile list into LDS as three 16-byte records {x, y, opacity, -} {conic a, b, c, -} {r, g, b, depth}.
// id = camera-major entry index c*U + g; an id outside the call reads as transparent (never the case for the forward's own sort).
// P has means2d, conics, colors, opac, comp, U and CU = C * U.  comp = the entries' antialiasing compensations [C,U] or null
// (classic: no load): the staged opacity is opac[g] * comp[id], one multiply, here and nowhere else, so both passes see one alpha.
template <class P>
__device__ __forceinline__ void stage_gaussian(const P& p, unsigned int id, int cam, f32x4* dst) {
  f32x4 a = {0.f, 0.f, 0.f, 0.f}, c = a, col = a;
  const unsigned int gi = id - (unsigned int)cam * (unsigned int)p.U;
  if (id < p.CU && gi < (unsigned int)p.U) {
    float o = p.opac[gi];
    if (p.comp) o *= p.comp[id];
    a = f32x4{p.means2d[2L * id], p.means2d[2L * id + 1], o, 0.f};
    c = f32x4{p.conics[3L * id], p.conics[3L * id + 1], p.conics[3L * id + 2], 0.f};
    col = *(const f32x4*)(p.colors + 4L * id);
  }
  dst[0] = a; dst[1] = c; dst[2] = col;
}

// Pixel (px, py) against the Gaussian of records a, c: ex = exp(-sigma), alpha = min(0.999, opacity * ex); false = the pair is
// skipped.  The one place that decides it: both passes must see the same alpha.
__host__ __device__ __forceinline__ bool pair_alpha(const f32x4& a, const f32x4& c, float px, float py, float& ex, float& alpha) {
  const float dx = a[0] - px, dy = a[1] - py;
  const float sigma = 0.5f * (c[0] * dx * dx + c[2] * dy * dy) + c[1] * dx * dy;
  ex = fast_exp(-sigma);
  alpha = fminf(0.999f, a[2] * ex);
  return !(sigma < 0.f || alpha < 1.f / 255.f);
}

// Front-to-back compositing of the tile list ids[s, e) by one 256-lane workgroup, a pixel per lane; s_g = 256 * 3 records of LDS.
// Leaves the pixel's transmittance T, the first NCH of its channels acc (r, g, b, depth; no background, no clamp) and the list
// index it stopped at (e if it ran through).  P as for stage_gaussian, plus ids.  An output the caller ignores costs nothing.
template <int NCH, class P>
__device__ __forceinline__ void composite_walk(const P& p, f32x4* s_g, int cam, unsigned int s, unsigned int e, float px, float py,
                                               bool inside, float& T, float* acc, unsigned int& stop) {
  const int tid = threadIdx.x;
  T = 1.f;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) acc[ch] = 0.f;
  stop = inside ? e : s;
  bool done = !inside;
  for (unsigned int base = s; base < e; base += 256) {
    if (__syncthreads_and(done)) break;  // also the barrier that protects s_g from the previous round's readers
    const unsigned int n = min(256u, e - base);
    if ((unsigned int)tid < n) stage_gaussian(p, p.ids[base + tid], cam, s_g + 3 * tid);
    __syncthreads();
    if (!done) {
      for (unsigned int k = 0; k < n; ++k) {
        float ex, alpha;
        if (!pair_alpha(s_g[3 * k], s_g[3 * k + 1], px, py, ex, alpha)) continue;
        const float nT = T * (1.f - alpha);
        if (nT <= 1e-4f) { done = true; stop = base + k; break; }
        const float vis = alpha * T;
        const f32x4 col = s_g[3 * k + 2];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) acc[ch] += col[ch] * vis;
        T = nT;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------- host-side checks
inline bool dims_ok(long U, int C, int width, int height, long max_isect) {
  if (U <= 0 || C <= 0 || width <= 0 || height <= 0 || max_isect <= 0 || max_isect >= (1L << 31)) return false;
  return U * (long)C < (1L << 32) && (long)tile_grid(width, height).ntiles * C < (1L << 24);
}

// the shape / SH arguments v3a_gs_project and v3a_gs_project_backward share: V3A_OK or the code to return
template <class A>
int check_sh_args(const A& a) {
  if (a.U < 0 || a.C <= 0 || a.width <= 0 || a.height <= 0 || a.U >= (1L << 31)) return V3A_ERR_SHAPE;
  if (a.sh_degree < 0 || a.sh_degree > 4 || a.sh_k < (a.sh_degree + 1) * (a.sh_degree + 1) || a.sh_k > 64) return V3A_ERR_SHAPE;
  if (a.sh_layout != 0 && a.sh_layout != 1) return V3A_ERR_ARG;
  if (a.rasterize_mode != 0 && a.rasterize_mode != 1) return V3A_ERR_ARG;
  return V3A_OK;
}

// f(std::integral_constant<int, deg>) for deg in 0..4 (checked by check_sh_args)
template <class F>
void dispatch_sh_degree(int deg, F&& f) {
  switch (deg) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

// f(degree as above, std::bool_constant<antialiased>): rasterize_mode 0 or 1 (checked by check_sh_args).  The mode is a template
// argument of the backward projection kernel so that its classic instantiations hold no trace of the other one.
template <class F>
void dispatch_sh_degree_mode(int deg, int mode, F&& f) {
  dispatch_sh_degree(deg, [&](auto d) {
    if (mode) f(d, std::true_type{});
    else f(d, std::false_type{});
  });
}

// The projection kernels of both directions: one wave per 64 Gaussians, their SH rows (3 * sh_k floats each) in dynamic LDS
template <class K, class P>
void launch_sh_waves(K kernel, const P& p, hipStream_t stream) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((p.U + 63) / 64)), dim3(64), (size_t)64 * 3 * p.sh_k * sizeof(float), stream, p);
}

}  // namespace gs
