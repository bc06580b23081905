// Backward of the 3D-Gaussian rasteriser (raster.hip) for gfx950, fp32: what gsplat's rasterize_to_pixels_bwd +
// fully_fused_projection_bwd + spherical_harmonics_bwd give torch.autograd, for the same call the forward replaces
// (RGB+D, classic or antialiased, packed=False, explicit world covariances).  Gradients reach means, covars, sh and opacities; cameras are
// constants unless v3a_gs_project_backward_cam is called, which also returns dL/d(viewmat, campos).
//
//   v3a_gs_rasterize_backward   count + rocPRIM scan (the forward's, re-run: each camera-Gaussian entry's first row slot) ->
//                               gs_blend_bwd_kernel, one 256-lane workgroup per 16x16 tile of every camera: walks the tile's
//                               list front to back exactly as the forward does to find every pixel's final T and stop index,
//                               then back to front; the ten per-pixel terms of a Gaussian are summed over the wave with DPP,
//                               over the four waves through LDS, and the (Gaussian, tile) row leaves the workgroup ONCE, with
//                               plain stores, to slot  first(entry) + tile's position inside the entry's tile rectangle ->
//                               gs_rowsum_kernel adds an entry's rows in slot order.
//   v3a_gs_project_backward     one wave per 64 Gaussians looping over the cameras in index order (as the forward): conic ->
//                               2D covariance -> J, camera covariance -> world covariance; mean through J, the pixel mean,
//                               the depth channel and the SH view direction; SH coefficients.  Antialiased mode: the entry's
//                               dL/d(opacity * comp) splits into the opacity's share (x comp) and dL/dcomp (x opacity), which
//                               enters the 2D covariance's gradient beside the conic's; comp is recomputed, not read.
//   v3a_gs_project_backward_cam the kernel above for the four Gaussian gradients (the same bits), then its CAM instantiation, which
//                               writes camera partials only: per camera, every lane's 15 terms of dL/d(R, t, campos) go to
//                               fp64, are summed over the wave (DPP, wave_sum's order) into one partial row [C, n_waves, 15] ->
//                               gs_cam_finish_kernel, one workgroup per camera: partials in index order, block_sum, ONE rounding to f32.
// No atomics on floats anywhere: every sum has a fixed order, results are bit-identical run to run.
#include "common.h"
#include "fixed_sum.h"
#include "gs_raster.h"
#include "../../include/vist3a_hip.h"

namespace {

using namespace gs;

constexpr int ROWF = 12;  // floats per row: d_means2d (2) d_conics (3) d_colors (4) d_opacity (1), then |d_means2d| (2) with ABS, else padding: three 16-byte stores
constexpr int BB = 128;   // Gaussians per backward round (4 waves x BB x 48 B of LDS partials)

__host__ __device__ __forceinline__ float fast_rcp(float x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_rcpf(x);
#else
  return 1.f / x;
#endif
}

// One pixel x one Gaussian of the back-to-front walk.  In: T = transmittance BEHIND this Gaussian (updated to the one in front),
// S[4] = colour accumulated behind it (updated), g[4] = dL/d(rgb, depth) of the pixel, gT = dL/dT_final, Tfin.  Out: the ten terms.
__host__ __device__ __forceinline__ void blend_bwd_pair(float dx, float dy, float ca, float cb, float cc, float opac, float ex, float alpha,
                                                        const f32x4& col, const float* g, float gT, float Tfin, float& T, float* S,
                                                        float* v) {
  const float ra = fast_rcp(1.f - alpha);
  T *= ra;
  const float vis = alpha * T;
  float va = -Tfin * ra * gT;
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) {
    v[5 + ch] = vis * g[ch];
    va += (col[ch] * T - S[ch] * ra) * g[ch];
    S[ch] += col[ch] * vis;
  }
  const float raw = opac * ex;
  if (raw <= 0.999f) {  // clamp_max passes the gradient only below the cap
    const float vs = -raw * va;
    v[0] = vs * (ca * dx + cb * dy);
    v[1] = vs * (cb * dx + cc * dy);
    v[2] = 0.5f * vs * dx * dx;
    v[3] = vs * dx * dy;
    v[4] = 0.5f * vs * dy * dy;
    v[9] = ex * va;
  } else {
    v[0] = v[1] = v[2] = v[3] = v[4] = v[9] = 0.f;
  }
}

// ---------------------------------------------------------------------------------------------- blend backward
struct BlendBwdP {
  const int* radii; const float* means2d; const float* conics; const float* colors; const float* opac; const float* comp;
  const unsigned int* offs; const unsigned int* ids; const unsigned int* counts; const unsigned int* incl;
  const float* bg; const float* d_color; const float* d_depth; const float* d_alpha;
  float* rows;
  unsigned int n_isect, CU;
  int U, W, H, tw, th, ntiles, clamp_rgb;
};

// wave_sum of common.h without the final broadcast: lane 63 holds the sum (the only lane that stores it)
__device__ __forceinline__ float wave_sum_lane63(float v) {
  v += dpp_f32<0xB1>(0.f, v);
  v += dpp_f32<0x4E>(0.f, v);
  v += dpp_f32<0x141>(0.f, v);
  v += dpp_f32<0x140>(0.f, v);
  v += dpp_f32<0x142, 0xA>(0.f, v);
  v += dpp_f32<0x143, 0xC>(0.f, v);
  return v;
}

// row slot of entry `id` in tile (tx, ty): the entry's rows are its tile rectangle in row-major order; ~0u = not a valid pair
__device__ __forceinline__ unsigned int row_slot(const BlendBwdP& p, unsigned int id, int tx, int ty) {
  if (id >= p.CU) return ~0u;
  const int r = p.radii[id];
  if (r <= 0) return ~0u;
  int x0, x1, y0, y1;
  tile_bounds(p.means2d[2L * id], p.means2d[2L * id + 1], r, p.tw, p.th, x0, x1, y0, y1);
  if (tx < x0 || tx >= x1 || ty < y0 || ty >= y1) return ~0u;
  const unsigned int slot = p.incl[id] - p.counts[id] + (unsigned int)((ty - y0) * (x1 - x0) + (tx - x0));
  return slot < p.n_isect ? slot : ~0u;
}

// ABS: the row's two spare floats carry the sums of |v[0]|, |v[1]| (gsplat's absgrad) through the same DPP, LDS and slot order.
template <bool ABS>
__global__ __launch_bounds__(256) void gs_blend_bwd_kernel(BlendBwdP p) {
  __shared__ f32x4 s_g[256 * 3];        // stage_gaussian's records
  __shared__ f32x4 s_part[4][BB][3];    // per wave, per Gaussian of the round: the ten reduced terms
  __shared__ unsigned int s_slot[BB];
  __shared__ unsigned int s_stop;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cam = blockIdx.x / p.ntiles, tile = blockIdx.x - cam * p.ntiles;
  const int tx = tile % p.tw, ty = tile / p.tw;
  const int px_i = tx * TILE + (tid & 15), py_i = ty * TILE + (tid >> 4);
  const bool inside = px_i < p.W && py_i < p.H;
  const float px = (float)px_i + 0.5f, py = (float)py_i + 0.5f;
  const unsigned int e = min(p.offs[blockIdx.x + 1], p.n_isect), s = min(p.offs[blockIdx.x], e);
  if (tid == 0) s_stop = s;

  // ---- front to back, the forward's walk: final T, pre-clamp colour, and the list index this pixel stopped at
  float T, acc[3];
  unsigned int stop;
  composite_walk<3>(p, s_g, cam, s, e, px, py, inside, T, acc, stop);
  float r = acc[0], g = acc[1], b = acc[2];
  // incoming gradients of this pixel; the clamp passes them where the un-clamped value lies in [0, 1], as torch.clamp does
  float gr[4] = {0.f, 0.f, 0.f, 0.f}, gT = 0.f;
  const float Tfin = T;
  if (inside) {
    const long pix = ((long)cam * p.H + py_i) * p.W + px_i;
    if (p.bg) { r += T * p.bg[0]; g += T * p.bg[1]; b += T * p.bg[2]; }
    gr[0] = p.d_color[3 * pix]; gr[1] = p.d_color[3 * pix + 1]; gr[2] = p.d_color[3 * pix + 2];
    if (p.clamp_rgb) {
      if (!(r >= 0.f && r <= 1.f)) gr[0] = 0.f;
      if (!(g >= 0.f && g <= 1.f)) gr[1] = 0.f;
      if (!(b >= 0.f && b <= 1.f)) gr[2] = 0.f;
    }
    gr[3] = p.d_depth[pix];
    gT = -p.d_alpha[pix];
    if (p.bg) gT += gr[0] * p.bg[0] + gr[1] * p.bg[1] + gr[2] * p.bg[2];
  }
  __syncthreads();
  atomicMax(&s_stop, stop);  // integer maximum in LDS: order-independent
  __syncthreads();
  const unsigned int wg_stop = s_stop;  // no pixel of the tile went past this list index

  // ---- back to front
  float S[4] = {0.f, 0.f, 0.f, 0.f};
  const int nround = (int)((wg_stop - s + BB - 1) / BB);
  for (int rd = nround - 1; rd >= 0; --rd) {
    const unsigned int base = s + (unsigned int)rd * BB;
    const int n = (int)min((unsigned int)BB, wg_stop - base);
    __syncthreads();  // the previous round's readers of s_g / s_part / s_slot
    if (tid < n) {
      const unsigned int id = p.ids[base + tid];
      stage_gaussian(p, id, cam, s_g + 3 * tid);
      s_slot[tid] = row_slot(p, id, tx, ty);
    }
    __syncthreads();
    for (int k = n - 1; k >= 0; --k) {
      const f32x4 a = s_g[3 * k], c = s_g[3 * k + 1];
      float ex, alpha;
      const bool valid = pair_alpha(a, c, px, py, ex, alpha) && (base + (unsigned int)k < stop);
      f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = o0, o2 = o0;
      if (__any(valid)) {  // wave-uniform: a wave is four pixel rows, most Gaussians touch few of them
        float v[10];
#pragma unroll
        for (int i = 0; i < 10; ++i) v[i] = 0.f;
        if (valid) blend_bwd_pair(a[0] - px, a[1] - py, c[0], c[1], c[2], a[2], ex, alpha, s_g[3 * k + 2], gr, gT, Tfin, T, S, v);
        [[maybe_unused]] const float ab0 = fabsf(v[0]), ab1 = fabsf(v[1]);   // this pixel's terms, before the sums
#pragma unroll
        for (int i = 0; i < 10; ++i) v[i] = wave_sum_lane63(v[i]);
        o0 = f32x4{v[0], v[1], v[2], v[3]}; o1 = f32x4{v[4], v[5], v[6], v[7]}; o2 = f32x4{v[8], v[9], 0.f, 0.f};
        if constexpr (ABS) { o2[2] = wave_sum_lane63(ab0); o2[3] = wave_sum_lane63(ab1); }
      }
      if (lane == 63) { s_part[wave][k][0] = o0; s_part[wave][k][1] = o1; s_part[wave][k][2] = o2; }
    }
    __syncthreads();
    if (tid < n) {
      const unsigned int slot = s_slot[tid];
      if (slot != ~0u) {
        f32x4 q[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) q[j] = ((s_part[0][tid][j] + s_part[1][tid][j]) + s_part[2][tid][j]) + s_part[3][tid][j];
        f32x4* dst = (f32x4*)(p.rows + (size_t)slot * ROWF);
        dst[0] = q[0]; dst[1] = q[1]; dst[2] = q[2];
      }
    }
  }
  // pairs behind the last stop were never composited: their rows are zero (every row slot is written exactly once, no memset)
  for (unsigned int i = wg_stop + tid; i < e; i += 256) {
    const unsigned int slot = row_slot(p, p.ids[i], tx, ty);
    if (slot != ~0u) {
      f32x4* dst = (f32x4*)(p.rows + (size_t)slot * ROWF);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      dst[0] = z; dst[1] = z; dst[2] = z;
    }
  }
}

struct RowSumP {
  const unsigned int* counts; const unsigned int* incl; const float* rows;
  long CU;
  unsigned int n_isect;
  float* d_means2d; float* d_conics; float* d_colors; float* d_opac; float* d_abs;
};

// one lane per camera-Gaussian entry: its rows in slot order (tile rectangle, row-major)
template <bool ABS>
__global__ __launch_bounds__(256) void gs_rowsum_kernel(RowSumP p) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= p.CU) return;
  const unsigned int cnt = p.counts[e], first = p.incl[e] - cnt;
  f32x4 q0 = {0.f, 0.f, 0.f, 0.f}, q1 = q0, q2 = q0;
  if (first <= p.n_isect && cnt <= p.n_isect - first) {
    const f32x4* src = (const f32x4*)(p.rows + (size_t)first * ROWF);
    for (unsigned int i = 0; i < cnt; ++i) { q0 += src[3 * i]; q1 += src[3 * i + 1]; q2 += src[3 * i + 2]; }
  }
  p.d_means2d[2 * e] = q0[0]; p.d_means2d[2 * e + 1] = q0[1];
  p.d_conics[3 * e] = q0[2]; p.d_conics[3 * e + 1] = q0[3]; p.d_conics[3 * e + 2] = q1[0];
  *(f32x4*)(p.d_colors + 4 * e) = f32x4{q1[1], q1[2], q1[3], q2[0]};
  p.d_opac[e] = q2[1];
  if constexpr (ABS) { p.d_abs[2 * e] = q2[2]; p.d_abs[2 * e + 1] = q2[3]; }
}

struct BLayout { size_t counts, incl, rows, tmp, tmp_bytes, total; };

BLayout blayout(long CU, long cap) {
  BLayout l{};
  size_t off = 0;
  auto take = [&](size_t b) { size_t o = off; off += align256(b); return o; };
  l.counts = take(4 * (size_t)CU); l.incl = take(4 * (size_t)CU);
  l.rows = take(sizeof(float) * ROWF * (size_t)cap);
  l.tmp_bytes = scan_tmp_bytes(CU);
  l.tmp = take(l.tmp_bytes);
  l.total = off;
  return l;
}

// ---------------------------------------------------------------------------------------------- projection backward
// Reverse of sh_eval: gk[k] = dL/d(basis k) -> dL/d(x, y, z) of the unit direction.
template <int DEG>
__host__ __device__ __forceinline__ void sh_eval_bwd(float x, float y, float z, const float* gk, float& vx, float& vy, float& vz) {
  vx = vy = vz = 0.f;
  if constexpr (DEG >= 1) { vy += -0.48860251190292f * gk[1]; vz += 0.48860251190292f * gk[2]; vx += -0.48860251190292f * gk[3]; }
  if constexpr (DEG >= 2) {
    const float z2 = z * z, t0b = -1.092548430592079f * z, c1 = x * x - y * y, s1 = 2.f * x * y;
    float v_z2 = 0.f, v_c1 = 0.f, v_s1 = 0.f, v_p6 = 0.f;
    if constexpr (DEG >= 3) {
      const float t0c = -2.285228997322329f * z2 + 0.4570457994644658f, t1b = 1.445305721320277f * z;
      const float c2 = x * c1 - y * s1, s2 = x * s1 + y * c1;
      float v_c2 = 0.f, v_s2 = 0.f, v_p12 = 0.f;
      if constexpr (DEG >= 4) {
        const float p12 = z * (1.865881662950577f * z2 - 1.119528997770346f);
        const float t0d = z * (-4.683325804901025f * z2 + 2.007139630671868f), t1c = 3.31161143515146f * z2 - 0.47308734787878f;
        const float t2b = -1.770130769779931f * z;
        const float v_s3 = 0.6258357354491763f * gk[16], v_c3 = 0.6258357354491763f * gk[24];
        const float v_t2b = gk[17] * s2 + gk[23] * c2;
        v_s2 += gk[17] * t2b; v_c2 += gk[23] * t2b;
        const float v_t1c = gk[18] * s1 + gk[22] * c1;
        v_s1 += gk[18] * t1c; v_c1 += gk[22] * t1c;
        const float v_t0d = gk[19] * y + gk[21] * x;
        vy += gk[19] * t0d; vx += gk[21] * t0d;
        vz += 1.984313483298443f * p12 * gk[20]; v_p12 += 1.984313483298443f * z * gk[20]; v_p6 += -1.006230589874905f * gk[20];
        vx += c2 * v_c3; v_c2 += x * v_c3; vy += -s2 * v_c3; v_s2 += -y * v_c3;   // c3 = x c2 - y s2
        vx += s2 * v_s3; v_s2 += x * v_s3; vy += c2 * v_s3; v_c2 += y * v_s3;    // s3 = x s2 + y c2
        vz += (-4.683325804901025f * z2 + 2.007139630671868f) * v_t0d; v_z2 += -4.683325804901025f * z * v_t0d;
        v_z2 += 3.31161143515146f * v_t1c;
        vz += -1.770130769779931f * v_t2b;
      }
      v_s2 += -0.5900435899266435f * gk[9]; v_c2 += -0.5900435899266435f * gk[15];
      const float v_t1b = gk[10] * s1 + gk[14] * c1;
      v_s1 += gk[10] * t1b; v_c1 += gk[14] * t1b;
      const float v_t0c = gk[11] * y + gk[13] * x;
      vy += gk[11] * t0c; vx += gk[13] * t0c;
      v_p12 += gk[12];
      vx += c1 * v_c2; v_c1 += x * v_c2; vy += -s1 * v_c2; v_s1 += -y * v_c2;    // c2 = x c1 - y s1
      vx += s1 * v_s2; v_s1 += x * v_s2; vy += c1 * v_s2; v_c1 += y * v_s2;     // s2 = x s1 + y c1
      vz += (1.865881662950577f * z2 - 1.119528997770346f) * v_p12; v_z2 += 1.865881662950577f * z * v_p12;
      v_z2 += -2.285228997322329f * v_t0c;
      vz += 1.445305721320277f * v_t1b;
    }
    v_s1 += 0.5462742152960395f * gk[4]; v_c1 += 0.5462742152960395f * gk[8];
    const float v_t0b = gk[5] * y + gk[7] * x;
    vy += gk[5] * t0b; vx += gk[7] * t0b;
    v_p6 += gk[6];
    v_z2 += 0.9461746957575601f * v_p6;
    vx += 2.f * y * v_s1; vy += 2.f * x * v_s1;
    vx += 2.f * x * v_c1; vy += -2.f * y * v_c1;
    vz += -1.092548430592079f * v_t0b;
    vz += 2.f * z * v_z2;
  }
}

struct ProjGeo {  // what the forward derives from the call's constants
  const float* V; const float* Kc; const float* campos;
  float W, H, eps2d;
};

// One visible (camera, Gaussian) entry.  m = world mean, sw = upper triangle of the world covariance (00 01 02 11 12 22),
// s = this Gaussian's SH row, vm2 / vcon / vcol = the entry's incoming gradients.  Adds into vm[3], vS[6] (symmetric dL/dS of the
// full matrix, same packing) and dsh[3 * NB] (basis-major: dsh[3 k + channel]).  AA (antialiased mode): vop_eff = the entry's
// dL/d(effective opacity), opac = the Gaussian's opacity; returns comp, and dL/dcomp = vop_eff * opac joins the conic's dL/dQ.
// CAM: also WRITES the entry's 15 camera terms to cam: [0..8] dL/dR (row-major) = v_c m^T + 2 W R S, [9..11] dL/dt = v_c (the
// camera-space mean gradient), [12..14] dL/dcampos = -dL/dd (the SH view direction; 0 where |d| < 1e-20, as the means' term).
template <int DEG, bool AA, bool CAM = false>
__host__ __device__ __forceinline__ float proj_bwd_entry(const ProjGeo& q, const float* m, const float* sw, const float* s, int sh_layout,
                                                         int sh_k, const float* vm2, const float* vcon, const float* vcol, float vop_eff,
                                                         float opac, float* vm, float* vS, float* dsh, float* cam = nullptr) {
  constexpr int NB = (DEG + 1) * (DEG + 1);
  const float* V = q.V;
  const float R00 = V[0], R01 = V[1], R02 = V[2], R10 = V[4], R11 = V[5], R12 = V[6], R20 = V[8], R21 = V[9], R22 = V[10];
  const float mx = m[0], my = m[1], mz = m[2];
  // the forward's chain up to the 2D covariance
  float x, y, z;
  to_camera(V, mx, my, mz, x, y, z);
  const ProjEntry e = project_entry<AA>(V, q.Kc, q.W, q.H, q.eps2d, x, y, z, sw[0], sw[1], sw[2], sw[3], sw[4], sw[5]);
  const float rz = e.rz, rz2 = e.rz2, fx = e.fx, fy = e.fy, tx = e.tx, ty = e.ty;
  const float lxp = e.lxp, lxn = e.lxn, lyp = e.lyp, lyn = e.lyn, j00 = e.j00, j02 = e.j02, j11 = e.j11, j12 = e.j12;
  const float t00 = e.t00, t01 = e.t01, t02 = e.t02, t10 = e.t10, t11 = e.t11, t12 = e.t12;
  const float xz = x * rz, yz = y * rz;
  const float cxz = fminf(lxp, fmaxf(-lxn, xz)), cyz = fminf(lyp, fmaxf(-lyn, yz));  // tx = z * cxz, ty = z * cyz
  const float id = 1.f / e.det;
  const float X00 = e.q11 * id, X01 = -e.q01 * id, X11 = e.q00 * id;  // the conic
  // conic = Q^-1:  dL/dQ = -X G X with G = [[va, vb/2], [vb/2, vc]]  (symmetric 2x2; M01 stands for both off-diagonal positions)
  const float G00 = vcon[0], G01 = 0.5f * vcon[1], G11 = vcon[2];
  const float h00 = X00 * G00 + X01 * G01, h01 = X00 * G01 + X01 * G11, h10 = X01 * G00 + X11 * G01, h11 = X01 * G01 + X11 * G11;
  float M00 = -(h00 * X00 + h01 * X01), M01 = -(h00 * X01 + h01 * X11), M11 = -(h10 * X01 + h11 * X11);
  float comp = 1.f;
  if constexpr (AA) {
    // comp = sqrt(r), r = det(Q - eps I) / det(Q):  dr/dQ = (1 - r) X - eps det(X) I,  dcomp/dQ = dr/dQ / (2 comp); exactly 0 at comp == 0
    float r;
    comp = compensation(e, r);
    if (comp > 0.f) {
      const float k = (vop_eff * opac) / (2.f * comp), omr = 1.f - r, ed = q.eps2d * id;  // det(X) = 1 / det(Q)
      M00 += k * (omr * X00 - ed); M01 += k * (omr * X01); M11 += k * (omr * X11 - ed);
    }
  }
  // Q = J Cc J^T + eps:  dL/dCc = J^T M J (symmetric 3x3),  dL/dJ = 2 M (J Cc)
  const float w00 = j00 * j00 * M00, w01 = j00 * j11 * M01, w02 = j00 * (M00 * j02 + M01 * j12);
  const float w11 = j11 * j11 * M11, w12 = j11 * (M01 * j02 + M11 * j12);
  const float w22 = j02 * j02 * M00 + 2.f * j02 * j12 * M01 + j12 * j12 * M11;
  const float vj00 = 2.f * (M00 * t00 + M01 * t10), vj02 = 2.f * (M00 * t02 + M01 * t12);
  const float vj11 = 2.f * (M01 * t01 + M11 * t11), vj12 = 2.f * (M01 * t02 + M11 * t12);
  // Cc = R S R^T:  dL/dS = R^T W R
  const float b00 = w00 * R00 + w01 * R10 + w02 * R20, b01 = w00 * R01 + w01 * R11 + w02 * R21, b02 = w00 * R02 + w01 * R12 + w02 * R22;
  const float b10 = w01 * R00 + w11 * R10 + w12 * R20, b11 = w01 * R01 + w11 * R11 + w12 * R21, b12 = w01 * R02 + w11 * R12 + w12 * R22;
  const float b20 = w02 * R00 + w12 * R10 + w22 * R20, b21 = w02 * R01 + w12 * R11 + w22 * R21, b22 = w02 * R02 + w12 * R12 + w22 * R22;
  vS[0] += R00 * b00 + R10 * b10 + R20 * b20; vS[1] += R00 * b01 + R10 * b11 + R20 * b21; vS[2] += R00 * b02 + R10 * b12 + R20 * b22;
  vS[3] += R01 * b01 + R11 * b11 + R21 * b21; vS[4] += R01 * b02 + R11 * b12 + R21 * b22;
  vS[5] += R02 * b02 + R12 * b12 + R22 * b22;
  // J, the pixel mean and the depth channel -> camera-space mean
  float vrz = fx * vj00 + fy * vj11 - 2.f * rz * (fx * tx * vj02 + fy * ty * vj12) + fx * x * vm2[0] + fy * y * vm2[1];
  const float vtx = -fx * rz2 * vj02, vty = -fy * rz2 * vj12;
  float vx = fx * rz * vm2[0], vy = fy * rz * vm2[1], vz = cxz * vtx + cyz * vty + vcol[3];
  if (xz >= -lxn && xz <= lxp) { vx += rz * z * vtx; vrz += x * z * vtx; }   // inside the clamp: tx = z * (x rz)
  if (yz >= -lyn && yz <= lyp) { vy += rz * z * vty; vrz += y * z * vty; }
  vz -= rz2 * vrz;
  vm[0] += R00 * vx + R10 * vy + R20 * vz; vm[1] += R01 * vx + R11 * vy + R21 * vz; vm[2] += R02 * vx + R12 * vy + R22 * vz;
  if constexpr (CAM) {  // mc = R m + t,  Cc = R S R^T:  dL/dt = v_c,  dL/dR = v_c m^T + 2 (W R) S  (b = W R from above)
    const float s00 = sw[0], s01 = sw[1], s02 = sw[2], s11 = sw[3], s12 = sw[4], s22 = sw[5];
    const float cx = vx, cy = vy, cz = vz, ox = mx, oy = my, oz = mz;
    const float d00 = b00, d01 = b01, d02 = b02, d10 = b10, d11 = b11, d12 = b12;
    const float d20 = b20, d21 = b21, d22 = b22;
    cam[0] = cx * ox + 2.f * (d00 * s00 + d01 * s01 + d02 * s02);
    cam[1] = cx * oy + 2.f * (d00 * s01 + d01 * s11 + d02 * s12);
    cam[2] = cx * oz + 2.f * (d00 * s02 + d01 * s12 + d02 * s22);
    cam[3] = cy * ox + 2.f * (d10 * s00 + d11 * s01 + d12 * s02);
    cam[4] = cy * oy + 2.f * (d10 * s01 + d11 * s11 + d12 * s12);
    cam[5] = cy * oz + 2.f * (d10 * s02 + d11 * s12 + d12 * s22);
    cam[6] = cz * ox + 2.f * (d20 * s00 + d21 * s01 + d22 * s02);
    cam[7] = cz * oy + 2.f * (d20 * s01 + d21 * s11 + d22 * s12);
    cam[8] = cz * oz + 2.f * (d20 * s02 + d21 * s12 + d22 * s22);
    cam[9] = cx; cam[10] = cy; cam[11] = cz;
  }
  // SH colour: clamp_min(c + 0.5, 0) mask, coefficients, and the view direction
  const float dx = mx - q.campos[0], dy = my - q.campos[1], dz = mz - q.campos[2];
  const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
  const float inv = 1.f / fmaxf(nrm, 1e-20f);
  const float ux = dx * inv, uy = dy * inv, uz = dz * inv;
  float bas[NB];
  sh_eval<DEG>(ux, uy, uz, bas);
  float r, gg, b;
  sh_color<DEG>(bas, s, sh_layout, sh_k, r, gg, b);
  const float vr = (r + 0.5f >= 0.f) ? vcol[0] : 0.f, vg = (gg + 0.5f >= 0.f) ? vcol[1] : 0.f, vb = (b + 0.5f >= 0.f) ? vcol[2] : 0.f;
  float gk[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    dsh[3 * k] += bas[k] * vr; dsh[3 * k + 1] += bas[k] * vg; dsh[3 * k + 2] += bas[k] * vb;
    gk[k] = (sh_layout == 0) ? s[3 * k] * vr + s[3 * k + 1] * vg + s[3 * k + 2] * vb : s[k] * vr + s[sh_k + k] * vg + s[2 * sh_k + k] * vb;
  }
  float vux, vuy, vuz;
  sh_eval_bwd<DEG>(ux, uy, uz, gk, vux, vuy, vuz);
  const float dot = ux * vux + uy * vuy + uz * vuz;  // u = d / |d|:  dL/dd = (v - u (u . v)) / |d|
  if (nrm >= 1e-20f) { vm[0] += (vux - ux * dot) * inv; vm[1] += (vuy - uy * dot) * inv; vm[2] += (vuz - uz * dot) * inv; }
  if constexpr (CAM) {  // d = m - campos
    const bool far = nrm >= 1e-20f;
    const float ax = vux, ay = vuy, az = vuz, ex = ux, ey = uy, ez = uz;
    const float od = dot, oi = inv;
    cam[12] = far ? -((ax - ex * od) * oi) : 0.f; cam[13] = far ? -((ay - ey * od) * oi) : 0.f;
    cam[14] = far ? -((az - ez * od) * oi) : 0.f;
  }
  return comp;
}

struct ProjBwdP {
  const float* means; const float* covars; const float* sh;
  const float* viewmat; const float* campos; const float* K;
  int sh_layout, sh_k;
  int U, C, W, H;
  float eps2d;
  const int* radii; const float* d_means2d; const float* d_conics; const float* d_colors; const float* d_opac;
  const float* opac;  // antialiased mode only: [U]
  float* d_means; float* d_covars; float* d_sh; float* d_opacities;
};

constexpr int NCAM = 15;  // camera terms of an entry: dL/dR (9), dL/dt (3), dL/dcampos (3)

struct ProjBwdCamP : ProjBwdP {
  double* part;  // out [C, n_waves, NCAM]: the waves' fp64 sums, n_waves = the grid
};

// v from the lane the DPP control names, +0.0 where it names none (or the row is masked off): dpp_f32 on the two halves of a double
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ double dpp_f64(double v) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned int lo = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)(unsigned int)b, CTRL, ROW_MASK, 0xF, false);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)(unsigned int)(b >> 32), CTRL, ROW_MASK, 0xF, false);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// wave_sum_lane63 in fp64, the same order: quads, half rows, rows, rows 0+1 / 2+3, halves.  All 64 lanes must be active.
__device__ __forceinline__ double wave_sum_lane63_f64(double v) {
  v += dpp_f64<0xB1>(v);
  v += dpp_f64<0x4E>(v);
  v += dpp_f64<0x141>(v);
  v += dpp_f64<0x140>(v);
  v += dpp_f64<0x142, 0xA>(v);
  v += dpp_f64<0x143, 0xC>(v);
  return v;
}

// One wave = 64 consecutive Gaussians, cameras in index order.  LDS: the SH rows of the 64 Gaussians (as the forward stages them),
// overwritten at the end by their gradient rows for a coalesced store.
// CAM (v3a_gs_project_backward_cam) is a body of its own, so that the other instantiations hold no trace of it (see project_entry
// in gs_raster.h for why): no lane leaves the camera loop - a culled entry and a lane past U carry 15 exact zeros - because the
// wave sums each camera's terms one at a time (fp32 -> fp64 is exact) and lane 63 stores the partial row.  It writes the camera
// partials ONLY: its own sums for means / covars / sh come out of hipcc with other fma contractions than the plain instantiation's
// (measured: last bits differ), so the entry point gets the four Gaussian gradients from the plain kernel, bit for bit, and this
// one drops them (dead code; the SH accumulators go, and with them most of the registers).
template <int DEG, bool AA, bool CAM = false>
__global__ __launch_bounds__(64) void gs_project_bwd_kernel(std::conditional_t<CAM, ProjBwdCamP, ProjBwdP> p) {
  extern __shared__ float s_sh[];
  constexpr int NB = (DEG + 1) * (DEG + 1);
  const int lane = threadIdx.x;
  const int g0 = blockIdx.x * 64;
  const int g = g0 + lane;
  const int row = 3 * p.sh_k;
  const int nrow = min(64, p.U - g0);
  const int total = nrow * row;
  stage_sh_rows(s_sh, p.sh + (long)g0 * row, total, lane);
  __syncthreads();
  float* s = s_sh + lane * row;
  if constexpr (CAM) {
    const bool live = g < p.U;
    const int gl = live ? g : p.U - 1;  // a lane past U reads the last Gaussian's scalars and uses none of them
    float vm[3] = {0.f, 0.f, 0.f}, vS[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // proj_bwd_entry's Gaussian sums: unused here, dead code
    float dsh[3 * NB];
#pragma unroll
    for (int i = 0; i < 3 * NB; ++i) dsh[i] = 0.f;
    const float m[3] = {p.means[3L * gl], p.means[3L * gl + 1], p.means[3L * gl + 2]};
    const float* cv = p.covars + 9L * gl;
    const float sw[6] = {cv[0], cv[1], cv[2], cv[4], cv[5], cv[8]};
    float opac = 0.f;
    if constexpr (AA) opac = p.opac[gl];
    for (int c = 0; c < p.C; ++c) {
      const long o = (long)c * p.U + gl;
      float cam[NCAM];
#pragma unroll
      for (int k = 0; k < NCAM; ++k) cam[k] = 0.f;
      if (live && p.radii[o] > 0) {
        const ProjGeo q = {p.viewmat + 16 * c, p.K + 9 * c, p.campos + 3 * c, (float)p.W, (float)p.H, p.eps2d};
        const float vm2[2] = {p.d_means2d[2 * o], p.d_means2d[2 * o + 1]};
        const float vcon[3] = {p.d_conics[3 * o], p.d_conics[3 * o + 1], p.d_conics[3 * o + 2]};
        const f32x4 vc4 = *(const f32x4*)(p.d_colors + 4 * o);
        const float vcol[4] = {vc4[0], vc4[1], vc4[2], vc4[3]};
        const float vo = p.d_opac[o];
        proj_bwd_entry<DEG, AA, true>(q, m, sw, s, p.sh_layout, p.sh_k, vm2, vcon, vcol, vo, opac, vm, vS, dsh, cam);
      }
      double* dst = p.part + ((size_t)c * gridDim.x + blockIdx.x) * NCAM;
#pragma unroll
      for (int k = 0; k < NCAM; ++k) {
        const double t = wave_sum_lane63_f64((double)cam[k]);
        if (lane == 63) dst[k] = t;
      }
    }
    return;  // the Gaussian gradients are the other instantiation's: nothing of d_means / d_covars / d_sh / d_opacities is written here
  } else if (g < p.U) {
    float vm[3] = {0.f, 0.f, 0.f}, vS[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, vop = 0.f;
    float dsh[3 * NB];
#pragma unroll
    for (int i = 0; i < 3 * NB; ++i) dsh[i] = 0.f;
    const float m[3] = {p.means[3L * g], p.means[3L * g + 1], p.means[3L * g + 2]};
    const float* cv = p.covars + 9L * g;
    const float sw[6] = {cv[0], cv[1], cv[2], cv[4], cv[5], cv[8]};
    float opac = 0.f;
    if constexpr (AA) opac = p.opac[g];
    for (int c = 0; c < p.C; ++c) {
      const long o = (long)c * p.U + g;
      if (p.radii[o] <= 0) continue;  // culled entries contribute exactly zero
      const ProjGeo q = {p.viewmat + 16 * c, p.K + 9 * c, p.campos + 3 * c, (float)p.W, (float)p.H, p.eps2d};
      const float vm2[2] = {p.d_means2d[2 * o], p.d_means2d[2 * o + 1]};
      const float vcon[3] = {p.d_conics[3 * o], p.d_conics[3 * o + 1], p.d_conics[3 * o + 2]};
      const f32x4 vc4 = *(const f32x4*)(p.d_colors + 4 * o);
      const float vcol[4] = {vc4[0], vc4[1], vc4[2], vc4[3]};
      const float vo = p.d_opac[o];
      const float comp = proj_bwd_entry<DEG, AA>(q, m, sw, s, p.sh_layout, p.sh_k, vm2, vcon, vcol, vo, opac, vm, vS, dsh);
      if constexpr (AA) vop += vo * comp;
      else vop += vo;
    }
    p.d_means[3L * g] = vm[0]; p.d_means[3L * g + 1] = vm[1]; p.d_means[3L * g + 2] = vm[2];
    float* dc = p.d_covars + 9L * g;  // "the upper triangle is used": an off-diagonal entry carries both symmetric positions
    dc[0] = vS[0]; dc[1] = 2.f * vS[1]; dc[2] = 2.f * vS[2];
    dc[3] = 0.f; dc[4] = vS[3]; dc[5] = 2.f * vS[4];
    dc[6] = 0.f; dc[7] = 0.f; dc[8] = vS[5];
    p.d_opacities[g] = vop;
    // this lane's SH row -> its gradient row (only this lane reads or writes row `lane`)
    for (int i = 0; i < row; ++i) s[i] = 0.f;
    if (p.sh_layout == 0) {
#pragma unroll
      for (int k = 0; k < NB; ++k) { s[3 * k] = dsh[3 * k]; s[3 * k + 1] = dsh[3 * k + 1]; s[3 * k + 2] = dsh[3 * k + 2]; }
    } else {
#pragma unroll
      for (int k = 0; k < NB; ++k) { s[k] = dsh[3 * k]; s[p.sh_k + k] = dsh[3 * k + 1]; s[2 * p.sh_k + k] = dsh[3 * k + 2]; }
    }
  }
  __syncthreads();
  float* dst = p.d_sh + (long)g0 * row;
  for (int i = lane; i < total; i += 64) dst[i] = s_sh[i];
}

struct CamFinishP { const double* part; int n_waves; float* d_viewmat; float* d_campos; };

// One workgroup per camera: lane t adds the partial rows t, t + 256, ... in index order, block_sum over the lanes, one rounding.
// Every element of d_viewmat [C,4,4] (bottom row: zeros) and d_campos [C,3] is written, nothing is memset.
__global__ __launch_bounds__(256) void gs_cam_finish_kernel(CamFinishP p) {
  __shared__ double red[256];
  const int c = blockIdx.x, tid = threadIdx.x;
  const double* src = p.part + (size_t)c * p.n_waves * NCAM;
  double acc[NCAM];
#pragma unroll
  for (int k = 0; k < NCAM; ++k) acc[k] = 0.0;
  for (int w = tid; w < p.n_waves; w += 256) {
#pragma unroll
    for (int k = 0; k < NCAM; ++k) acc[k] += src[(size_t)w * NCAM + k];
  }
  float* vmat = p.d_viewmat + 16 * c;
#pragma unroll
  for (int k = 0; k < NCAM; ++k) {
    const float t = (float)block_sum<256>(acc[k], red);
    if (tid == 0) {
      if (k < 9) vmat[4 * (k / 3) + k % 3] = t;        // dL/dR
      else if (k < 12) vmat[4 * (k - 9) + 3] = t;      // dL/dt
      else p.d_campos[3 * c + (k - 12)] = t;
    }
  }
  if (tid < 4) vmat[12 + tid] = 0.f;
}

inline long cam_waves(long U) { return (U + 63) / 64; }

}  // namespace

extern "C" long v3a_gs_rasterize_backward_workspace_bytes(long U, int C, int width, int height, long max_isect) {
  if (!dims_ok(U, C, width, height, max_isect)) return V3A_ERR_SHAPE;
  return (long)blayout(U * C, max_isect).total;
}

extern "C" int v3a_gs_rasterize_backward(const v3a_gs_rasterize_backward_args* a, void* stream_) {
  if (!a || !a->radii || !a->means2d || !a->conics || !a->colors || !a->opacities || !a->tile_offsets || !a->d_color || !a->d_depth ||
      !a->d_alpha || !a->d_means2d || !a->d_conics || !a->d_colors || !a->d_opacity_partial || !a->workspace)
    return V3A_ERR_ARG;
  if (a->n_isect < 0 || (a->n_isect > 0 && !a->flatten_ids)) return V3A_ERR_ARG;
  if (!dims_ok(a->U, a->C, a->width, a->height, a->n_isect > 0 ? a->n_isect : 1)) return V3A_ERR_SHAPE;
  hipStream_t stream = (hipStream_t)stream_;
  const TileGrid tg = tile_grid(a->width, a->height);
  const long CU = a->U * a->C;
  const BLayout l = blayout(CU, a->n_isect > 0 ? a->n_isect : 1);
  if ((size_t)a->workspace_bytes < l.total) return V3A_ERR_WORKSPACE;
  char* ws = (char*)a->workspace;
  unsigned int* counts = (unsigned int*)(ws + l.counts);
  unsigned int* incl = (unsigned int*)(ws + l.incl);
  float* rows = (float*)(ws + l.rows);
  const unsigned gb = (unsigned)((CU + 255) / 256);
  if (!count_and_scan({a->radii, a->means2d, CU, tg.tw, tg.th, counts}, incl, ws + l.tmp, l.tmp_bytes, stream)) return V3A_ERR_LAUNCH;
  BlendBwdP bp = {a->radii, a->means2d, a->conics, a->colors, a->opacities, a->compensations, a->tile_offsets, a->flatten_ids, counts, incl, a->background,
                  a->d_color, a->d_depth, a->d_alpha, rows, (unsigned int)a->n_isect, (unsigned int)CU, (int)a->U, a->width, a->height,
                  tg.tw, tg.th, tg.ntiles, a->clamp_rgb};
  const dim3 bgrid((unsigned)(tg.ntiles * a->C));
  RowSumP rp = {counts, incl, rows, CU, (unsigned int)a->n_isect, a->d_means2d, a->d_conics, a->d_colors, a->d_opacity_partial, a->d_means2d_abs};
  if (a->d_means2d_abs) {
    if (a->n_isect > 0) hipLaunchKernelGGL(gs_blend_bwd_kernel<true>, bgrid, dim3(256), 0, stream, bp);
    hipLaunchKernelGGL(gs_rowsum_kernel<true>, dim3(gb), dim3(256), 0, stream, rp);
  } else {
    if (a->n_isect > 0) hipLaunchKernelGGL(gs_blend_bwd_kernel<false>, bgrid, dim3(256), 0, stream, bp);
    hipLaunchKernelGGL(gs_rowsum_kernel<false>, dim3(gb), dim3(256), 0, stream, rp);
  }
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_gs_project_backward(const v3a_gs_project_backward_args* a, void* stream) {
  if (!a || !a->means || !a->covars || !a->sh || !a->viewmat || !a->campos || !a->K || !a->radii || !a->d_means2d || !a->d_conics ||
      !a->d_colors || !a->d_opacity_partial || !a->d_means || !a->d_covars || !a->d_sh || !a->d_opacities)
    return V3A_ERR_ARG;
  if (const int rc = check_sh_args(*a)) return rc;
  if (a->rasterize_mode == 1 && !a->opacities) return V3A_ERR_ARG;
  if (a->U == 0) return V3A_OK;
  ProjBwdP p = {a->means, a->covars, a->sh, a->viewmat, a->campos, a->K, a->sh_layout, a->sh_k, (int)a->U, a->C, a->width, a->height,
                a->eps2d, a->radii, a->d_means2d, a->d_conics, a->d_colors, a->d_opacity_partial, a->opacities, a->d_means, a->d_covars, a->d_sh,
                a->d_opacities};
  dispatch_sh_degree_mode(a->sh_degree, a->rasterize_mode, [&](auto d, auto aa) {
    launch_sh_waves(gs_project_bwd_kernel<decltype(d)::value, decltype(aa)::value>, p, (hipStream_t)stream);
  });
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" long v3a_gs_project_backward_cam_workspace_bytes(long U, int C) {
  if (U < 0 || C <= 0 || U >= (1L << 31)) return V3A_ERR_SHAPE;
  return (long)(sizeof(double) * NCAM * (size_t)cam_waves(U) * (size_t)C);
}

extern "C" int v3a_gs_project_backward_cam(const v3a_gs_project_backward_args* a, float* d_viewmat, float* d_campos, void* workspace,
                                           long workspace_bytes, void* stream) {
  if (!a || !a->means || !a->covars || !a->sh || !a->viewmat || !a->campos || !a->K || !a->radii || !a->d_means2d || !a->d_conics ||
      !a->d_colors || !a->d_opacity_partial || !a->d_means || !a->d_covars || !a->d_sh || !a->d_opacities || !d_viewmat || !d_campos ||
      !workspace)
    return V3A_ERR_ARG;
  if (const int rc = check_sh_args(*a)) return rc;
  if (a->rasterize_mode == 1 && !a->opacities) return V3A_ERR_ARG;
  if (((uintptr_t)workspace & 7) != 0) return V3A_ERR_ARG;
  if (workspace_bytes < v3a_gs_project_backward_cam_workspace_bytes(a->U, a->C)) return V3A_ERR_WORKSPACE;
  ProjBwdCamP p = {{a->means, a->covars, a->sh, a->viewmat, a->campos, a->K, a->sh_layout, a->sh_k, (int)a->U, a->C, a->width, a->height,
                    a->eps2d, a->radii, a->d_means2d, a->d_conics, a->d_colors, a->d_opacity_partial, a->opacities, a->d_means, a->d_covars,
                    a->d_sh, a->d_opacities},
                   (double*)workspace};
  if (a->U > 0)
    dispatch_sh_degree_mode(a->sh_degree, a->rasterize_mode, [&](auto d, auto aa) {
      launch_sh_waves(gs_project_bwd_kernel<decltype(d)::value, decltype(aa)::value>, static_cast<const ProjBwdP&>(p), (hipStream_t)stream);
      launch_sh_waves(gs_project_bwd_kernel<decltype(d)::value, decltype(aa)::value, true>, p, (hipStream_t)stream);
    });
  const CamFinishP f = {p.part, (int)cam_waves(a->U), d_viewmat, d_campos};  // U == 0: no partials, exact zeros
  hipLaunchKernelGGL(gs_cam_finish_kernel, dim3((unsigned)a->C), dim3(256), 0, (hipStream_t)stream, f);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
