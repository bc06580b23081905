// 3D-Gaussian rasteriser for gfx950 — the step right after the text->3DGS path.
// Replaces gsplat==1.4.0 `rasterization(..., render_mode="RGB+D", packed=False, rasterize_mode="classic", covars=...)` as
// called one camera at a time by /root/reference/third_party_model/anysplat/src/model/decoder/decoder_splatting_cuda.py:96-125.
//
//   v3a_gs_project    one wave per 64 Gaussians, ALL C cameras of the batch: the 64 x 300-B SH block is staged once into
//                     LDS with coalesced 16-B loads (it is 75 % of the input bytes) and mean/covariance are held in
//                     registers while the wave loops over cameras: world->camera, EWA projection of the 3x3 covariance,
//                     +eps2d blur, conic, 3-sigma radius, near/far/screen culling, SH colour for survivors.  With
//                     rasterize_mode 1 (gsplat's "antialiased") a second small kernel writes the opacity compensation of
//                     every entry, which v3a_gs_rasterize multiplies into the opacity as it stages a Gaussian.
//   v3a_gs_rasterize  tile counts -> rocPRIM scan -> (camera | tile | depth bits) keys -> rocPRIM stable radix sort ->
//                     tile ranges -> one 256-lane workgroup per 16x16 tile of every camera (C x tiles workgroups fill the
//                     256 CUs where one camera's ~800 tiles cannot): Gaussians staged through LDS 256 at a time, read back
//                     as wave-uniform 16-B broadcasts, front-to-back compositing with workgroup-wide early exit.
// The reference renders one camera per gsplat call (decoder_splatting_cuda.py:96); batching cameras is the same arithmetic
// per camera and is what keeps an MI355X busy.
//
// HBM-bound integer/byte work up to the blend; the blend is VALU-bound (one v_exp_f32 per pixel-Gaussian pair).  Index work
// (tile bounds, keys, order, ranges) is bit-exact against oracle/gsplat_raster.py; pixel values agree to fp32 tolerance.
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>

#include "common.h"
#include "gs_raster.h"
#include "../../include/vist3a_hip.h"

namespace {

using namespace gs;  // the forward math, shared with raster_bwd.hip

struct ProjP {
  const float* means; const float* covars; const float* sh;
  const float* viewmat; const float* campos; const float* K;
  int sh_layout, sh_k, sh_degree;
  int U, C, W, H;
  float near_plane, far_plane, radius_clip, eps2d;
  int* radii; float* means2d; float* depths; float* conics; float* colors;
};

// One wave = 64 consecutive Gaussians.  LDS image of their SH block: rows of 3*sh_k floats, lane l reads row l (odd row
// pitch for the production sh_k = 25 -> conflict-free ds_read_b32).
template <int DEG>
__global__ __launch_bounds__(64) void gs_project_kernel(ProjP p) {
  extern __shared__ float s_sh[];
  constexpr int NB = (DEG + 1) * (DEG + 1);
  const int lane = threadIdx.x;
  const int g0 = blockIdx.x * 64;
  const int g = g0 + lane;
  const int row = 3 * p.sh_k;
  const int nrow = min(64, p.U - g0);
  stage_sh_rows(s_sh, p.sh + (long)g0 * row, nrow * row, lane);
  __syncthreads();
  if (g >= p.U) return;
  const float mx = p.means[3L * g], my = p.means[3L * g + 1], mz = p.means[3L * g + 2];
  const float* cv = p.covars + 9L * g;  // upper triangle of the symmetric world covariance
  const float s00 = cv[0], s01 = cv[1], s02 = cv[2], s11 = cv[4], s12 = cv[5], s22 = cv[8];
  const float* s = s_sh + lane * row;
  const float W = (float)p.W, H = (float)p.H;
  for (int c = 0; c < p.C; ++c) {
    const float* V = p.viewmat + 16 * c;
    float x, y, z;
    to_camera(V, mx, my, mz, x, y, z);
    const long o = (long)c * p.U + g;
    int radius_i = 0;
    float m2x = 0.f, m2y = 0.f, ca = 0.f, cb = 0.f, cc = 0.f;
    if (z >= p.near_plane && z <= p.far_plane) {
      const ProjEntry e = project_entry(V, p.K + 9 * c, W, H, p.eps2d, x, y, z, s00, s01, s02, s11, s12, s22);
      m2x = e.fx * e.x * e.rz + e.cx;
      m2y = e.fy * e.y * e.rz + e.cy;
      if (e.det > 0.f) {
        const float id = 1.f / e.det;
        ca = e.q11 * id; cb = -e.q01 * id; cc = e.q00 * id;
        const float mid = 0.5f * (e.q00 + e.q11);
        const float v1 = mid + sqrtf(fmaxf(0.01f, mid * mid - e.det));
        const float radius = ceilf(3.f * sqrtf(v1));
        const bool off = (m2x + radius <= 0.f) || (m2x - radius >= W) || (m2y + radius <= 0.f) || (m2y - radius >= H);
        if (radius > p.radius_clip && !off) radius_i = (int)radius;
      }
    }
    p.radii[o] = radius_i;
    p.depths[o] = z;
    p.means2d[2 * o] = m2x; p.means2d[2 * o + 1] = m2y;
    p.conics[3 * o] = ca; p.conics[3 * o + 1] = cb; p.conics[3 * o + 2] = cc;
    float r = 0.f, gg = 0.f, b = 0.f;
    if (radius_i > 0) {  // SH colour only for Gaussians that will be drawn (gsplat's `masks = radii > 0`)
      float dx = mx - p.campos[3 * c], dy = my - p.campos[3 * c + 1], dz = mz - p.campos[3 * c + 2];
      const float n = sqrtf(dx * dx + dy * dy + dz * dz);
      const float inv = 1.f / fmaxf(n, 1e-20f);
      float bas[NB];
      sh_eval<DEG>(dx * inv, dy * inv, dz * inv, bas);
      sh_color<DEG>(bas, s, p.sh_layout, p.sh_k, r, gg, b);
      r = fmaxf(r + 0.5f, 0.f); gg = fmaxf(gg + 0.5f, 0.f); b = fmaxf(b + 0.5f, 0.f);
    }
    f32x4 col = {r, gg, b, z};
    *(f32x4*)(p.colors + 4 * o) = col;
  }
}

// Antialiased mode: the opacity compensation of every entry, 0 for a culled one.  A kernel of its own AFTER the classic projection
// (it reads that kernel's radii), one lane per Gaussian looping over the cameras with mean and covariance in registers: the mode's
// radii / means2d / conics / colours are then the classic kernel's by construction, bit for bit, and classic calls run what they
// always ran.  The price is a second read of means and covars (48 of the ~350 bytes per Gaussian the projection moves).
struct CompP {
  const float* means; const float* covars; const float* viewmat; const float* K; const int* radii;
  int U, C, W, H;
  float eps2d;
  float* comp;
};

__global__ __launch_bounds__(256) void gs_compensation_kernel(CompP p) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= p.U) return;
  const float mx = p.means[3L * g], my = p.means[3L * g + 1], mz = p.means[3L * g + 2];
  const float* cv = p.covars + 9L * g;
  const float s00 = cv[0], s01 = cv[1], s02 = cv[2], s11 = cv[4], s12 = cv[5], s22 = cv[8];
  for (int c = 0; c < p.C; ++c) {
    const long o = (long)c * p.U + g;
    float comp = 0.f;
    if (p.radii[o] > 0) {  // inside near / far and det > 0, or the projection would have culled it
      const float* V = p.viewmat + 16 * c;
      float x, y, z;
      to_camera(V, mx, my, mz, x, y, z);
      const ProjEntry e = project_entry<true>(V, p.K + 9 * c, (float)p.W, (float)p.H, p.eps2d, x, y, z, s00, s01, s02, s11, s12, s22);
      float r;
      comp = compensation(e, r);
    }
    p.comp[o] = comp;
  }
}

// ---------------------------------------------------------------------------------------------- binning
struct BinP {
  const int* radii; const float* means2d; const float* depths;
  long CU;  // C * U entries
  int U, tw, th;
  unsigned int* counts; unsigned int* incl;
  unsigned long long* keys; unsigned int* vals;
  unsigned int* offs;
  unsigned int n;
  int nt_all;  // C * tiles
};

__global__ __launch_bounds__(256) void gs_emit_kernel(BinP p) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= p.CU) return;
  const int r = p.radii[e];
  if (r <= 0) return;
  int x0, x1, y0, y1;
  tile_bounds(p.means2d[2 * e], p.means2d[2 * e + 1], r, p.tw, p.th, x0, x1, y0, y1);
  unsigned int o = p.incl[e] - p.counts[e];
  const unsigned long long cam_tile0 = (unsigned long long)(e / p.U) * (unsigned long long)(p.tw * p.th);
  const unsigned long long d = (unsigned long long)__float_as_uint(p.depths[e]);
  for (int i = y0; i < y1; ++i)
    for (int j = x0; j < x1; ++j) {
      p.keys[o] = ((cam_tile0 + (unsigned long long)(i * p.tw + j)) << 32) | d;
      p.vals[o] = (unsigned int)e;
      ++o;
    }
}

// offs[t] = first sorted intersection whose (camera, tile) id >= t, offs[C*ntiles] = n
__global__ __launch_bounds__(256) void gs_ranges_kernel(BinP p) {
  const unsigned int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p.n) return;
  const int t = (int)(p.keys[i] >> 32);
  const int prev = (i == 0) ? -1 : (int)(p.keys[i - 1] >> 32);
  for (int k = prev + 1; k <= t; ++k) p.offs[k] = i;
  if (i == p.n - 1)
    for (int k = t + 1; k <= p.nt_all; ++k) p.offs[k] = p.n;
}

// ---------------------------------------------------------------------------------------------- compositing
struct BlendP {
  const float* means2d; const float* conics; const float* colors; const float* opac; const float* comp;
  const unsigned int* offs; const unsigned int* ids;
  const float* bg;
  float* out_color; float* out_depth; float* out_alpha;
  unsigned int CU;
  int U, W, H, tw, ntiles, clamp_rgb;
};

__global__ __launch_bounds__(256) void gs_blend_kernel(BlendP p) {
  __shared__ f32x4 s_g[256 * 3];
  const int tid = threadIdx.x;
  const int cam = blockIdx.x / p.ntiles, tile = blockIdx.x - cam * p.ntiles;
  const int px_i = (tile % p.tw) * TILE + (tid & 15), py_i = (tile / p.tw) * TILE + (tid >> 4);
  const bool inside = px_i < p.W && py_i < p.H;
  float T, acc[4];
  unsigned int stop;
  composite_walk<4>(p, s_g, cam, p.offs[blockIdx.x], p.offs[blockIdx.x + 1], (float)px_i + 0.5f, (float)py_i + 0.5f, inside, T, acc, stop);
  if (!inside) return;
  float r = acc[0], g = acc[1], b = acc[2];
  if (p.bg) { r += T * p.bg[0]; g += T * p.bg[1]; b += T * p.bg[2]; }
  if (p.clamp_rgb) { r = fminf(fmaxf(r, 0.f), 1.f); g = fminf(fmaxf(g, 0.f), 1.f); b = fminf(fmaxf(b, 0.f), 1.f); }
  const long pix = ((long)cam * p.H + py_i) * p.W + px_i;
  p.out_color[3 * pix] = r; p.out_color[3 * pix + 1] = g; p.out_color[3 * pix + 2] = b;
  p.out_depth[pix] = acc[3];
  p.out_alpha[pix] = 1.f - T;
}

struct RLayout { size_t counts, incl, keys0, keys1, vals0, vals1, offs, tmp, tmp_bytes, total; };

RLayout rlayout(long CU, long nt_all, long cap) {
  RLayout l{};
  size_t off = 0;
  auto take = [&](size_t b) { size_t o = off; off += align256(b); return o; };
  l.counts = take(4 * (size_t)CU); l.incl = take(4 * (size_t)CU);
  l.keys0 = take(8 * (size_t)cap); l.keys1 = take(8 * (size_t)cap);
  l.vals0 = take(4 * (size_t)cap); l.vals1 = take(4 * (size_t)cap);
  l.offs = take(4 * (size_t)(nt_all + 1));
  size_t t1 = 0;
  (void)rocprim::radix_sort_pairs(nullptr, t1, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned int*)nullptr,
                                  (unsigned int*)nullptr, (size_t)cap, 0, 64);
  l.tmp_bytes = std::max(t1, scan_tmp_bytes(CU));
  l.tmp = take(l.tmp_bytes);
  l.total = off;
  return l;
}

}  // namespace

extern "C" int v3a_gs_project(const v3a_gs_project_args* a, void* stream) {
  if (!a || !a->means || !a->covars || !a->sh || !a->viewmat || !a->campos || !a->K || !a->radii || !a->means2d || !a->depths ||
      !a->conics || !a->colors)
    return V3A_ERR_ARG;
  if (const int rc = check_sh_args(*a)) return rc;
  if (a->rasterize_mode == 1 && !a->compensations) return V3A_ERR_ARG;
  if (a->U == 0) return V3A_OK;
  ProjP p = {a->means, a->covars, a->sh, a->viewmat, a->campos, a->K, a->sh_layout, a->sh_k, a->sh_degree, (int)a->U, a->C, a->width,
             a->height, a->near_plane, a->far_plane, a->radius_clip, a->eps2d, a->radii, a->means2d, a->depths, a->conics, a->colors};
  dispatch_sh_degree(a->sh_degree, [&](auto d) { launch_sh_waves(gs_project_kernel<decltype(d)::value>, p, (hipStream_t)stream); });
  if (a->rasterize_mode == 1) {
    CompP cp = {a->means, a->covars, a->viewmat, a->K, a->radii, (int)a->U, a->C, a->width, a->height, a->eps2d, a->compensations};
    hipLaunchKernelGGL(gs_compensation_kernel, dim3((unsigned)((a->U + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cp);
  }
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" long v3a_gs_rasterize_workspace_bytes(long U, int C, int width, int height, long max_isect) {
  if (!dims_ok(U, C, width, height, max_isect)) return V3A_ERR_SHAPE;
  return (long)rlayout(U * C, (long)tile_grid(width, height).ntiles * C, max_isect).total;
}

extern "C" int v3a_gs_rasterize(const v3a_gs_rasterize_args* a, void* stream_) {
  if (!a || !a->radii || !a->means2d || !a->depths || !a->conics || !a->colors || !a->opacities || !a->out_color || !a->out_depth ||
      !a->out_alpha || !a->workspace || !a->n_isect)
    return V3A_ERR_ARG;
  if (!dims_ok(a->U, a->C, a->width, a->height, a->max_isect)) return V3A_ERR_SHAPE;
  hipStream_t stream = (hipStream_t)stream_;
  const TileGrid tg = tile_grid(a->width, a->height);
  const long CU = a->U * a->C;
  const int nt_all = tg.ntiles * a->C;
  const RLayout l = rlayout(CU, nt_all, a->max_isect);
  if ((size_t)a->workspace_bytes < l.total) return V3A_ERR_SHAPE;
  char* ws = (char*)a->workspace;
  BinP b = {};
  b.radii = a->radii; b.means2d = a->means2d; b.depths = a->depths;
  b.CU = CU; b.U = (int)a->U; b.tw = tg.tw; b.th = tg.th; b.nt_all = nt_all;
  b.counts = (unsigned int*)(ws + l.counts); b.incl = (unsigned int*)(ws + l.incl);
  b.keys = (unsigned long long*)(ws + l.keys0); b.vals = (unsigned int*)(ws + l.vals0);
  b.offs = (unsigned int*)(ws + l.offs);
  const unsigned gb = (unsigned)((CU + 255) / 256);
  if (!count_and_scan({b.radii, b.means2d, CU, tg.tw, tg.th, b.counts}, b.incl, ws + l.tmp, l.tmp_bytes, stream)) return V3A_ERR_LAUNCH;
  // the intersection count sizes the sort: one 4-byte read-back per camera batch (gsplat does the same `.item()` per camera)
  unsigned int n = 0;
  if (hipMemcpyAsync(&n, b.incl + (CU - 1), 4, hipMemcpyDeviceToHost, stream) != hipSuccess) return V3A_ERR_LAUNCH;
  if (hipStreamSynchronize(stream) != hipSuccess) return V3A_ERR_LAUNCH;
  *a->n_isect = (long)n;
  if ((long)n > a->max_isect) return V3A_ERR_WORKSPACE;
  if (hipMemsetAsync(b.offs, 0, 4 * (size_t)(nt_all + 1), stream) != hipSuccess) return V3A_ERR_LAUNCH;
  const unsigned int* ids = b.vals;
  if (n > 0) {
    hipLaunchKernelGGL(gs_emit_kernel, dim3(gb), dim3(256), 0, stream, b);
    int tile_bits = 1;
    while ((1L << tile_bits) < nt_all) ++tile_bits;
    size_t tb = l.tmp_bytes;
    unsigned long long* k1 = (unsigned long long*)(ws + l.keys1);
    unsigned int* v1 = (unsigned int*)(ws + l.vals1);
    if (rocprim::radix_sort_pairs(ws + l.tmp, tb, b.keys, k1, b.vals, v1, (size_t)n, 0, 32 + tile_bits, stream) != hipSuccess)
      return V3A_ERR_LAUNCH;
    b.keys = k1; b.vals = v1; b.n = n;
    ids = v1;
    hipLaunchKernelGGL(gs_ranges_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, b);
  }
  if (a->tile_offsets_out &&
      hipMemcpyAsync(a->tile_offsets_out, b.offs, 4 * (size_t)(nt_all + 1), hipMemcpyDeviceToDevice, stream) != hipSuccess)
    return V3A_ERR_LAUNCH;
  if (a->flatten_ids_out && n > 0 &&
      hipMemcpyAsync(a->flatten_ids_out, ids, 4 * (size_t)n, hipMemcpyDeviceToDevice, stream) != hipSuccess)
    return V3A_ERR_LAUNCH;
  BlendP bp = {a->means2d, a->conics, a->colors, a->opacities, a->compensations, b.offs, ids, a->background, a->out_color, a->out_depth, a->out_alpha,
               (unsigned int)CU, (int)a->U, a->width, a->height, tg.tw, tg.ntiles, a->clamp_rgb};
  hipLaunchKernelGGL(gs_blend_kernel, dim3((unsigned)nt_all), dim3(256), 0, stream, bp);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
