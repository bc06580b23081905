// Post-optimisation of predicted Gaussians (third_party_model/anysplat/src/post_opt/simple_trainer.py): the two elementwise
// passes around the rasteriser and the photometric loss.
//
//   splat activation   (log-scales, raw quaternions xyzw, opacity logits) -> (covariances, opacities), forward and backward.
//                      What gsplat does inside its rasterisation call from exp(scales), quats, sigmoid(opacities)
//                      (simple_trainer.py:607-634); here the covariance is explicit because v3a_gs_project takes one.  Quaternion
//                      order, internal normalisation and the product are those of gaussian_adapter_kernel (elementwise.hip).
//   fused Adam         torch.optim.Adam's update on one parameter tensor per launch (simple_trainer.py:442-460: one optimiser per
//                      tensor, eps 1e-15), in place.
//   camera adjust      the pose optimiser's parametrisation (post_opt/utils.py:12-48, :117-138): 9 deltas per camera (translation +
//                      6D rotation) -> the adjusted view matrix and camera centre, forward and backward, in closed form (no matrix
//                      inverse on the device, nothing read back).
#include "common.h"
#include "splat_quat.h"   // quat_R: the rotation of a raw quaternion, shared with mcmc.hip
#include "../../include/vist3a_hip.h"

namespace {

// One thread per Gaussian: 8 floats in, 10 out; rows of adjacent lanes are adjacent in memory.
__global__ void __launch_bounds__(256) splat_activate_kernel(const float* __restrict__ log_scales, const float* __restrict__ quats,
                                                             const float* __restrict__ logits, long U, float* __restrict__ cov,
                                                             float* __restrict__ opac) {
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= U) return;
  float s[3], q[4], R[9];
#pragma unroll
  for (int e = 0; e < 3; ++e) s[e] = expf(log_scales[u * 3 + e]);
#pragma unroll
  for (int e = 0; e < 4; ++e) q[e] = quats[u * 4 + e];
  quat_R(q, R);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      float acc = 0.f;
#pragma unroll
      for (int m = 0; m < 3; ++m) acc += (R[a * 3 + m] * s[m]) * s[m] * R[b * 3 + m];
      cov[u * 9 + a * 3 + b] = acc;
    }
  opac[u] = 1.f / (1.f + expf(-logits[u]));
}

// Closed form.  With G = d_covars (any 3 x 3: v3a_gs_project_backward fills the upper triangle only and lets an off-diagonal entry
// carry both symmetric positions; autograd through C = R D R^T contracts G with dC entry by entry, and so does this):
//   dD_m = r_m^T G r_m (r_m = column m of R),  d log s_m = 2 s_m^2 dD_m,  dR = (G + G^T) R D,
// and R(q) = I + t M(q), t = 2 / |q|^2 (the normalisation cancels: R is invariant to the quaternion's length), so
//   dq_e = t sum_ab dR_ab dM_ab/dq_e - (2 t q_e / |q|^2) sum_ab dR_ab M_ab.
__global__ void __launch_bounds__(256) splat_activate_bwd_kernel(const float* __restrict__ log_scales, const float* __restrict__ quats,
                                                                 const float* __restrict__ logits, const float* __restrict__ d_cov,
                                                                 const float* __restrict__ d_opac, long U,
                                                                 float* __restrict__ d_log_scales, float* __restrict__ d_quats,
                                                                 float* __restrict__ d_logits) {
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= U) return;
  float s2[3], q[4], R[9], G[9];
#pragma unroll
  for (int e = 0; e < 3; ++e) { const float s = expf(log_scales[u * 3 + e]); s2[e] = s * s; }
#pragma unroll
  for (int e = 0; e < 4; ++e) q[e] = quats[u * 4 + e];
#pragma unroll
  for (int e = 0; e < 9; ++e) G[e] = d_cov[u * 9 + e];
  quat_R(q, R);
  float g[9];   // dR
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    float gr[3], dD = 0.f;   // (G + G^T) r_m
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      float acc = 0.f, accG = 0.f;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        acc += (G[a * 3 + b] + G[b * 3 + a]) * R[b * 3 + m];
        accG += G[a * 3 + b] * R[b * 3 + m];
      }
      gr[a] = acc;
      dD += R[a * 3 + m] * accG;
    }
    d_log_scales[u * 3 + m] = 2.f * s2[m] * dD;
#pragma unroll
    for (int a = 0; a < 3; ++a) g[a * 3 + m] = gr[a] * s2[m];
  }
  const float i = q[0], j = q[1], k = q[2], r = q[3];
  const float n2 = i * i + j * j + k * k + r * r;
  const float t = 2.f / n2;
  const float S = g[0] * -(j * j + k * k) + g[1] * (i * j - k * r) + g[2] * (i * k + j * r)
                + g[3] * (i * j + k * r) + g[4] * -(i * i + k * k) + g[5] * (j * k - i * r)
                + g[6] * (i * k - j * r) + g[7] * (j * k + i * r) + g[8] * -(i * i + j * j);
  const float di = j * (g[1] + g[3]) + k * (g[2] + g[6]) + r * (g[7] - g[5]) - 2.f * i * (g[4] + g[8]);
  const float dj = i * (g[1] + g[3]) + k * (g[5] + g[7]) + r * (g[2] - g[6]) - 2.f * j * (g[0] + g[8]);
  const float dk = i * (g[2] + g[6]) + j * (g[5] + g[7]) + r * (g[3] - g[1]) - 2.f * k * (g[0] + g[4]);
  const float dr = i * (g[7] - g[5]) + j * (g[2] - g[6]) + k * (g[3] - g[1]);
  const float c = 2.f * t / n2 * S;
  d_quats[u * 4 + 0] = t * di - c * i;
  d_quats[u * 4 + 1] = t * dj - c * j;
  d_quats[u * 4 + 2] = t * dk - c * k;
  d_quats[u * 4 + 3] = t * dr - c * r;
  const float o = 1.f / (1.f + expf(-logits[u]));
  d_logits[u] = d_opac[u] * o * (1.f - o);
}

struct AdamP {
  float* p; const float* g; float* m; float* v;
  long n, nvec;
  int period;              // > 0: element e uses step2 unless e % period == 0
  double b1, b2, step1, step2;
  float inv_sqrt_bc2, eps;
};

// The moments and the parameter are advanced in fp64 and rounded once on store (they are fp32 in memory): the kernel is bound by its
// 28 bytes per element, and m = b1 m + (1 - b1) g cancels when the gradient changes sign, where fp32 arithmetic loses digits.
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, double step, const AdamP& a) {
  const float mn = (float)(a.b1 * (double)m + (1.0 - a.b1) * (double)g);
  const float vn = (float)(a.b2 * (double)v + (1.0 - a.b2) * ((double)g * (double)g));
  const float upd = mn / (sqrtf(vn) * a.inv_sqrt_bc2 + a.eps);
  m = mn;
  v = vn;
  p = (float)((double)p - step * (double)upd);
}

__global__ void __launch_bounds__(256) adam_kernel(const AdamP a) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < a.nvec) {   // 16-byte loads and stores
    float4 p = ((const float4*)a.p)[t], m = ((const float4*)a.m)[t], v = ((const float4*)a.v)[t];
    const float4 g = ((const float4*)a.g)[t];
    double st[4];
    const unsigned r0 = a.period > 0 ? (unsigned)((t * 4) % a.period) : 0u;   // one 64-bit remainder per lane, the rest in 32 bits
#pragma unroll
    for (int e = 0; e < 4; ++e) st[e] = (a.period > 0 && (r0 + e) % (unsigned)a.period != 0) ? a.step2 : a.step1;
    adam_one(p.x, g.x, m.x, v.x, st[0], a);
    adam_one(p.y, g.y, m.y, v.y, st[1], a);
    adam_one(p.z, g.z, m.z, v.z, st[2], a);
    adam_one(p.w, g.w, m.w, v.w, st[3], a);
    ((float4*)a.p)[t] = p;
    ((float4*)a.m)[t] = m;
    ((float4*)a.v)[t] = v;
  } else {            // scalar tail (and the whole tensor when a pointer is not 16-byte aligned)
    const long e = a.nvec * 4 + (t - a.nvec);
    if (e >= a.n) return;
    float p = a.p[e], m = a.m[e], v = a.v[e];
    adam_one(p, a.g[e], m, v, (a.period > 0 && e % a.period != 0) ? a.step2 : a.step1, a);
    a.p[e] = p;
    a.m[e] = m;
    a.v[e] = v;
  }
}

// ---------------------------------------------------------------------------------------------- visibility-masked Adam
// The step's visibility mask: one thread per Gaussian walks the cameras in index order; every byte is written once.
__global__ void __launch_bounds__(256) gs_visibility_kernel(const int* __restrict__ radii, int C, long U, uint8_t* __restrict__ visible) {
  const long u = (long)blockIdx.x * 256 + threadIdx.x;
  if (u >= U) return;
  int seen = 0;
  for (int c = 0; c < C; ++c) seen |= radii[(long)c * U + u] > 0;
  visible[u] = (uint8_t)seen;
}

// gsplat's SelectiveAdam on rows of M floats: adam_kernel's flat map (thread t owns elements 4t .. 4t + 3 of the whole tensor, lane i
// at base + 16 i, so a wave's accesses stay one contiguous KiB whatever M is), with the mask looked up per element.  A thread whose
// four elements are all visible takes adam_kernel's 16-byte path; one with none returns before any load of p, g, m, v; a thread that
// straddles a visible and an invisible row goes element by element, so that an invisible row is neither loaded nor stored.  The
// arithmetic is adam_one with both bias corrections 1.
__global__ void __launch_bounds__(256) adam_visible_kernel(const AdamP a, const uint8_t* __restrict__ visible, const long M) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t < a.nvec) {
    const long e0 = t * 4;
    long row = e0 / M;
    long col = e0 - row * M;
    bool vis[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      vis[e] = visible[row] != 0;
      if (++col == M) { col = 0; ++row; }
    }
    const bool any = vis[0] | vis[1] | vis[2] | vis[3], all = vis[0] & vis[1] & vis[2] & vis[3];
    if (!any) return;
    double st[4];
    const unsigned r0 = a.period > 0 ? (unsigned)(e0 % a.period) : 0u;
#pragma unroll
    for (int e = 0; e < 4; ++e) st[e] = (a.period > 0 && (r0 + e) % (unsigned)a.period != 0) ? a.step2 : a.step1;
    if (all) {
      float4 p = ((const float4*)a.p)[t], m = ((const float4*)a.m)[t], v = ((const float4*)a.v)[t];
      const float4 g = ((const float4*)a.g)[t];
      adam_one(p.x, g.x, m.x, v.x, st[0], a);
      adam_one(p.y, g.y, m.y, v.y, st[1], a);
      adam_one(p.z, g.z, m.z, v.z, st[2], a);
      adam_one(p.w, g.w, m.w, v.w, st[3], a);
      ((float4*)a.p)[t] = p;
      ((float4*)a.m)[t] = m;
      ((float4*)a.v)[t] = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (!vis[e]) continue;
        float p = a.p[e0 + e], m = a.m[e0 + e], v = a.v[e0 + e];
        adam_one(p, a.g[e0 + e], m, v, st[e], a);
        a.p[e0 + e] = p;
        a.m[e0 + e] = m;
        a.v[e0 + e] = v;
      }
    }
  } else {            // scalar tail (and the whole tensor when a pointer is not 16-byte aligned)
    const long e = a.nvec * 4 + (t - a.nvec);
    if (e >= a.n || visible[e / M] == 0) return;
    float p = a.p[e], m = a.m[e], v = a.v[e];
    adam_one(p, a.g[e], m, v, (a.period > 0 && e % a.period != 0) ? a.step2 : a.step1, a);
    a.p[e] = p;
    a.m[e] = m;
    a.v[e] = v;
  }
}

// ---------------------------------------------------------------------------------------------- camera pose deltas
// The rotation of a 6D delta (utils.py:117-138): a1 = r[0..2] + (1,0,0), a2 = r[3..5] + (0,1,0); b1 = a1 / max(|a1|, 1e-12),
// u = a2 - (b1 . a2) b1, b2 = u / max(|u|, 1e-12), b3 = b1 x b2.  Rd has the ROWS b1, b2, b3.
struct Gram {
  double a2[3], b1[3], b2[3], b3[3], u[3], n1, nu, l1, lu, s;   // l = the norms, n = their clamped values, s = b1 . a2
};

__device__ __forceinline__ Gram gram_schmidt(const float* r) {
  Gram q;
  const double a1[3] = {(double)r[0] + 1.0, (double)r[1], (double)r[2]};
  q.a2[0] = (double)r[3]; q.a2[1] = (double)r[4] + 1.0; q.a2[2] = (double)r[5];
  q.l1 = sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
  q.n1 = fmax(q.l1, 1e-12);
  for (int i = 0; i < 3; ++i) q.b1[i] = a1[i] / q.n1;
  q.s = q.b1[0] * q.a2[0] + q.b1[1] * q.a2[1] + q.b1[2] * q.a2[2];
  for (int i = 0; i < 3; ++i) q.u[i] = q.a2[i] - q.s * q.b1[i];
  q.lu = sqrt(q.u[0] * q.u[0] + q.u[1] * q.u[1] + q.u[2] * q.u[2]);
  q.nu = fmax(q.lu, 1e-12);
  for (int i = 0; i < 3; ++i) q.b2[i] = q.u[i] / q.nu;
  q.b3[0] = q.b1[1] * q.b2[2] - q.b1[2] * q.b2[1];
  q.b3[1] = q.b1[2] * q.b2[0] - q.b1[0] * q.b2[2];
  q.b3[2] = q.b1[0] * q.b2[1] - q.b1[1] * q.b2[0];
  return q;
}

// c2w' = c2w_base [Rd | dx]  ->  viewmat = inverse(c2w') = [Rd^T | -Rd^T dx] w2c_base,  campos = c2w'[:3,3] = R_c2w dx + t_c2w.
// One thread per camera, fp64 after the loads, one rounding at the store.  A zero delta gives Rd = I exactly and every product
// below is by exactly 1 or 0: the outputs are then the base matrices.
__global__ void __launch_bounds__(64) camera_adjust_kernel(const float* __restrict__ w2c, const float* __restrict__ c2w,
                                                           const float* __restrict__ deltas, int V, float* __restrict__ viewmat,
                                                           float* __restrict__ campos) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= V) return;
  const float* d = deltas + 9 * c;
  const Gram q = gram_schmidt(d + 3);
  const double dx[3] = {(double)d[0], (double)d[1], (double)d[2]};
  const double* b[3] = {q.b1, q.b2, q.b3};
  const float* Wm = w2c + 16 * c;
  const float* Cm = c2w + 16 * c;
  for (int i = 0; i < 3; ++i) {
    // row i of [Rd^T | p]:  Rd^T[i][k] = b_k[i],  p = -Rd^T dx
    const double n0 = b[0][i], n1 = b[1][i], n2 = b[2][i];
    const double p = -(n0 * dx[0] + n1 * dx[1] + n2 * dx[2]);
    for (int j = 0; j < 4; ++j)
      viewmat[16 * c + 4 * i + j] =
          (float)(n0 * (double)Wm[j] + n1 * (double)Wm[4 + j] + n2 * (double)Wm[8 + j] + p * (double)Wm[12 + j]);
    campos[3 * c + i] = (float)((double)Cm[4 * i] * dx[0] + (double)Cm[4 * i + 1] * dx[1] + (double)Cm[4 * i + 2] * dx[2] + (double)Cm[4 * i + 3]);
  }
  for (int j = 0; j < 4; ++j) viewmat[16 * c + 12 + j] = Wm[12 + j];
}

// Backward of the above: (dL/dviewmat [V,4,4], dL/dcampos [V,3]) -> dL/ddeltas [V,9], every element written once, linear in the
// incoming gradients.  viewmat's bottom row is the base's: no gradient passes through it.
__global__ void __launch_bounds__(64) camera_adjust_bwd_kernel(const float* __restrict__ w2c, const float* __restrict__ c2w,
                                                               const float* __restrict__ deltas, const float* __restrict__ d_viewmat,
                                                               const float* __restrict__ d_campos, int V, float* __restrict__ d_deltas) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= V) return;
  const float* d = deltas + 9 * c;
  const Gram q = gram_schmidt(d + 3);
  const double dx[3] = {(double)d[0], (double)d[1], (double)d[2]};
  const float* Wm = w2c + 16 * c;
  const float* Cm = c2w + 16 * c;
  const float* G = d_viewmat + 16 * c;
  // A = [Rd^T | p] (top three rows):  dL/dA = G w2c^T
  double gA[3][4];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 4; ++k)
      gA[i][k] = (double)G[4 * i] * (double)Wm[4 * k] + (double)G[4 * i + 1] * (double)Wm[4 * k + 1] +
                 (double)G[4 * i + 2] * (double)Wm[4 * k + 2] + (double)G[4 * i + 3] * (double)Wm[4 * k + 3];
  // p = -Rd^T dx:  dL/d(Rd^T)[i][k] += -gp[i] dx[k],  dL/ddx = -Rd gp;  campos = R_c2w dx + t:  dL/ddx += R_c2w^T g_campos
  double gb[3][3];   // gb[k] = dL/db_k (row k of Rd):  Rd^T[i][k] = b_k[i]
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i) gb[k][i] = gA[i][k] - gA[i][3] * dx[k];
  const double* b[3] = {q.b1, q.b2, q.b3};
  const double gc[3] = {(double)d_campos[3 * c], (double)d_campos[3 * c + 1], (double)d_campos[3 * c + 2]};
  double out[9];
  for (int k = 0; k < 3; ++k)
    out[k] = -(b[k][0] * gA[0][3] + b[k][1] * gA[1][3] + b[k][2] * gA[2][3]) +
             ((double)Cm[k] * gc[0] + (double)Cm[4 + k] * gc[1] + (double)Cm[8 + k] * gc[2]);
  // b3 = b1 x b2:  dL/db1 += b2 x g3,  dL/db2 += g3 x b1
  const double* g3 = gb[2];
  gb[0][0] += q.b2[1] * g3[2] - q.b2[2] * g3[1]; gb[0][1] += q.b2[2] * g3[0] - q.b2[0] * g3[2]; gb[0][2] += q.b2[0] * g3[1] - q.b2[1] * g3[0];
  gb[1][0] += g3[1] * q.b1[2] - g3[2] * q.b1[1]; gb[1][1] += g3[2] * q.b1[0] - g3[0] * q.b1[2]; gb[1][2] += g3[0] * q.b1[1] - g3[1] * q.b1[0];
  // b2 = u / max(|u|, eps): the clamp passes the norm's gradient where |u| >= eps
  double gu[3];
  {
    const double dot = q.lu >= 1e-12 ? q.b2[0] * gb[1][0] + q.b2[1] * gb[1][1] + q.b2[2] * gb[1][2] : 0.0;
    for (int i = 0; i < 3; ++i) gu[i] = (gb[1][i] - q.b2[i] * dot) / q.nu;
  }
  // u = a2 - s b1, s = b1 . a2
  const double gs = -(gu[0] * q.b1[0] + gu[1] * q.b1[1] + gu[2] * q.b1[2]);
  for (int i = 0; i < 3; ++i) {
    out[6 + i] = gu[i] + gs * q.b1[i];
    gb[0][i] += -q.s * gu[i] + gs * q.a2[i];
  }
  {
    const double dot = q.l1 >= 1e-12 ? q.b1[0] * gb[0][0] + q.b1[1] * gb[0][1] + q.b1[2] * gb[0][2] : 0.0;
    for (int i = 0; i < 3; ++i) out[3 + i] = (gb[0][i] - q.b1[i] * dot) / q.n1;
  }
  for (int i = 0; i < 9; ++i) d_deltas[9 * c + i] = (float)out[i];
}

}  // namespace

extern "C" int v3a_camera_adjust(const float* w2c_base, const float* c2w_base, const float* deltas, int V, float* viewmat, float* campos,
                                 void* stream) {
  if (!w2c_base || !c2w_base || !deltas || !viewmat || !campos) return V3A_ERR_ARG;
  if (V < 1 || V > (1 << 24)) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(camera_adjust_kernel, dim3((unsigned)((V + 63) / 64)), dim3(64), 0, (hipStream_t)stream, w2c_base, c2w_base, deltas, V,
                     viewmat, campos);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_camera_adjust_backward(const float* w2c_base, const float* c2w_base, const float* deltas, const float* d_viewmat,
                                          const float* d_campos, int V, float* d_deltas, void* stream) {
  if (!w2c_base || !c2w_base || !deltas || !d_viewmat || !d_campos || !d_deltas) return V3A_ERR_ARG;
  if (V < 1 || V > (1 << 24)) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(camera_adjust_bwd_kernel, dim3((unsigned)((V + 63) / 64)), dim3(64), 0, (hipStream_t)stream, w2c_base, c2w_base, deltas,
                     d_viewmat, d_campos, V, d_deltas);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_splat_activate(const float* log_scales, const float* quats, const float* logits, long U, float* covars,
                                  float* opacities, void* stream) {
  if (!log_scales || !quats || !logits || !covars || !opacities) return V3A_ERR_ARG;
  if (U < 1 || U > 0x7fffffffL * 256) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(splat_activate_kernel, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, (hipStream_t)stream, log_scales, quats, logits,
                     U, covars, opacities);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_splat_activate_backward(const float* log_scales, const float* quats, const float* logits, const float* d_covars,
                                           const float* d_opacities, long U, float* d_log_scales, float* d_quats, float* d_logits,
                                           void* stream) {
  if (!log_scales || !quats || !logits || !d_covars || !d_opacities || !d_log_scales || !d_quats || !d_logits) return V3A_ERR_ARG;
  if (U < 1 || U > 0x7fffffffL * 256) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(splat_activate_bwd_kernel, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, (hipStream_t)stream, log_scales, quats,
                     logits, d_covars, d_opacities, U, d_log_scales, d_quats, d_logits);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_adam_step(const v3a_adam_args* a, void* stream) {
  if (!a || !a->p || !a->g || !a->m || !a->v) return V3A_ERR_ARG;
  if (a->n < 1 || a->period < 0 || !(a->bias_correction1 > 0.0) || !(a->bias_correction2 > 0.0)) return V3A_ERR_SHAPE;
  AdamP k;
  k.p = a->p; k.g = a->g; k.m = a->m; k.v = a->v;
  k.n = a->n;
  const uintptr_t al = (uintptr_t)a->p | (uintptr_t)a->g | (uintptr_t)a->m | (uintptr_t)a->v;
  k.nvec = (al & 15) ? 0 : a->n / 4;
  k.period = a->period;
  k.b1 = a->beta1;
  k.b2 = a->beta2;
  k.step1 = a->lr / a->bias_correction1;
  k.step2 = a->lr2 / a->bias_correction1;
  k.inv_sqrt_bc2 = (float)(1.0 / sqrt(a->bias_correction2));
  k.eps = (float)a->eps;
  const long threads = k.nvec + (a->n - 4 * k.nvec);
  if ((threads + 255) / 256 > 0x7fffffffL) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_gs_visibility(const int* radii, int C, long U, uint8_t* visible, void* stream) {
  if (!radii || !visible) return V3A_ERR_ARG;
  if (C < 1 || U < 1 || U > 0x7fffffffL * 256) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(gs_visibility_kernel, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, (hipStream_t)stream, radii, C, U, visible);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_adam_step_visible(const v3a_adam_visible_args* a, void* stream) {
  if (!a || !a->p || !a->g || !a->m || !a->v || !a->visible) return V3A_ERR_ARG;
  if (a->U < 1 || a->M < 1 || a->period < 0 || a->M > 0x7fffffffffffffffL / a->U) return V3A_ERR_SHAPE;
  AdamP k;
  k.p = a->p; k.g = a->g; k.m = a->m; k.v = a->v;
  k.n = a->U * a->M;
  const uintptr_t al = (uintptr_t)a->p | (uintptr_t)a->g | (uintptr_t)a->m | (uintptr_t)a->v;
  k.nvec = (al & 15) ? 0 : k.n / 4;
  k.period = a->period;
  k.b1 = a->beta1;
  k.b2 = a->beta2;
  k.step1 = a->lr;      // no bias correction: both are 1
  k.step2 = a->lr2;
  k.inv_sqrt_bc2 = 1.f;
  k.eps = (float)a->eps;
  const long threads = k.nvec + (k.n - 4 * k.nvec);
  if ((threads + 255) / 256 > 0x7fffffffL) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(adam_visible_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k, a->visible, a->M);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
