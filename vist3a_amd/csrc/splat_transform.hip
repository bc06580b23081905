// Similarity transforms of a scene, x' = s R x + t, on the strided views of splat_scene.h.  DESIGN.md section 7i states the contract.
// Three entry points:
//
//   v3a_splat_transform        one wave per 64 rows.  The rows' harmonics are staged through LDS (consecutive lanes on consecutive floats
//                              of a row: coalesced over strided rows, both ways); a lane then turns its own row, band by band, with the
//                              band matrices read as wave-uniform kernel arguments.  A row's LDS pitch is 3 (K + 1) | 1 floats: odd, so
//                              the 32 lanes of a half wave sit on 32 different banks (the pitches 12 and 48 of degree 1 and 3 would be
//                              4- and 16-way conflicts).  Where the pitch is the row itself (degree 0, 2, 4) and the rows are contiguous
//                              from a 16-byte boundary, the wave's block is one run and moves 16 bytes per lane.  Every row of the wave is read whole before any of it is written: in place
//                              (out == in, same strides) is allowed.  No atomics; a row's result does not depend on the launch shape.
//   v3a_sh_rotation_matrices   the band matrices D_l(R), l = 1..deg, in fp64 on the host (no device needed).
//   v3a_splat_moments          count, sum (x - c) and the six sums (x - c)(x - c)^T of strided means about a centre, in fp64: a lane adds
//                              its 4 rows of a 1024-row tile in index order, then block_sum (fixed_sum.h); one workgroup adds the tiles'
//                              partials tid, tid + 256, ... in index order, then block_sum.  The tiles depend on the row count alone.
//
// Arithmetic of the transform: fp32, every dot product one multiply followed by fmaf in index order (spelled out: nothing is left
// to contraction), on fp32 roundings of s R, t, log s, q_R and D_l, which the host computes in fp64.
#include "common.h"
#include "fixed_sum.h"
#include "splat_scene.h"
#include "../../include/vist3a_hip.h"

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int WAVE = 64;
constexpr int MAX_DEG = 4;
constexpr int N_COEF = 164;            // 3^2 + 5^2 + 7^2 + 9^2
constexpr int MOM_THREADS = 256, MOM_ITEMS = 4, MOM_TILE = MOM_THREADS * MOM_ITEMS, MOM_OUT = 10;

__host__ __device__ constexpr int band_offset(int l) { return l == 1 ? 0 : l == 2 ? 9 : l == 3 ? 34 : l == 4 ? 83 : N_COEF; }

// ------------------------------------------------------------------------------------------------ band matrices (host, fp64)

// sh_eval of gs_raster.h in fp64: the same polynomials, constants, component order and signs
void sh_eval64(double x, double y, double z, double* b) {
  b[0] = 0.2820947917738781;
  b[1] = -0.48860251190292 * y; b[2] = 0.48860251190292 * z; b[3] = -0.48860251190292 * x;
  const double z2 = z * z, t0b = -1.092548430592079 * z, c1 = x * x - y * y, s1 = 2. * x * y;
  const double p6 = 0.9461746957575601 * z2 - 0.3153915652525201;
  b[4] = 0.5462742152960395 * s1; b[5] = t0b * y; b[6] = p6; b[7] = t0b * x; b[8] = 0.5462742152960395 * c1;
  const double t0c = -2.285228997322329 * z2 + 0.4570457994644658, t1b = 1.445305721320277 * z;
  const double c2 = x * c1 - y * s1, s2 = x * s1 + y * c1;
  const double p12 = z * (1.865881662950577 * z2 - 1.119528997770346);
  b[9] = -0.5900435899266435 * s2; b[10] = t1b * s1; b[11] = t0c * y; b[12] = p12; b[13] = t0c * x; b[14] = t1b * c1;
  b[15] = -0.5900435899266435 * c2;
  const double t0d = z * (-4.683325804901025 * z2 + 2.007139630671868), t1c = 3.31161143515146 * z2 - 0.47308734787878;
  const double t2b = -1.770130769779931 * z, c3 = x * c2 - y * s2, s3 = x * s2 + y * c2;
  b[16] = 0.6258357354491763 * s3; b[17] = t2b * s2; b[18] = t1c * s1; b[19] = t0d * y;
  b[20] = 1.984313483298443 * z * p12 - 1.006230589874905 * p6;
  b[21] = t0d * x; b[22] = t1c * c1; b[23] = t2b * c2; b[24] = 0.6258357354491763 * c3;
}

void matmul3(const double* a, const double* b, double* c) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

double det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// a proper rotation to 1e-6: V3A_OK or V3A_ERR_ARG (a NaN fails the comparisons)
int check_rotation(const double* R) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double g = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1. : 0.);
      if (!(std::fabs(g) <= 1e-6)) return V3A_ERR_ARG;
    }
  return det3(R) > 0. ? V3A_OK : V3A_ERR_ARG;
}

// Two Newton steps towards the nearest orthogonal matrix, R <- R (3 I - R^T R) / 2: 1e-6 off becomes rounding error, and a matrix
// that is orthogonal already in fp64 - the identity, a quarter turn - stays as it is, bit for bit.
void polish_rotation(const double* R, double* P) {
  for (int i = 0; i < 9; ++i) P[i] = R[i];
  for (int it = 0; it < 2; ++it) {
    double Rt[9], G[9], N[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Rt[3 * i + j] = P[3 * j + i];
    matmul3(Rt, P, G);
    for (int i = 0; i < 9; ++i) G[i] = ((i % 4 == 0 ? 3. : 0.) - G[i]) * 0.5;
    matmul3(P, G, N);
    for (int i = 0; i < 9; ++i) P[i] = N[i];
  }
}

// The fixed sample directions of the fit: a Fibonacci spiral of 64 unit vectors
constexpr int N_DIR = 64;
void sample_direction(int k, double* d) {
  const double z = 1. - (2. * k + 1.) / N_DIR, r = std::sqrt(1. - z * z), phi = 2.399963229728653 * k;
  d[0] = r * std::cos(phi); d[1] = r * std::sin(phi); d[2] = z;
  const double n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  d[0] /= n; d[1] /= n; d[2] /= n;
}

// inverse of the n x n matrix m (n <= 9, symmetric positive definite here) by Gauss-Jordan with partial pivoting
bool invert(double* m, int n, double* inv) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) inv[i * n + j] = i == j ? 1. : 0.;
  for (int c = 0; c < n; ++c) {
    int p = c;
    for (int r = c + 1; r < n; ++r)
      if (std::fabs(m[r * n + c]) > std::fabs(m[p * n + c])) p = r;
    if (!(std::fabs(m[p * n + c]) > 1e-12)) return false;
    for (int j = 0; j < n; ++j) { std::swap(m[c * n + j], m[p * n + j]); std::swap(inv[c * n + j], inv[p * n + j]); }
    const double d = 1. / m[c * n + c];
    for (int j = 0; j < n; ++j) { m[c * n + j] *= d; inv[c * n + j] *= d; }
    for (int r = 0; r < n; ++r) {
      if (r == c) continue;
      const double f = m[r * n + c];
      if (f == 0.) continue;
      for (int j = 0; j < n; ++j) { m[r * n + j] -= f * m[c * n + j]; inv[r * n + j] -= f * inv[c * n + j]; }
    }
  }
  return true;
}

// D_l(R), l = 1..deg, row-major, band after band (band_offset), of an orthogonal R: the least-squares fit of
// Y_l(R d_k) = D_l Y_l(d_k) over the sample directions, solved for the DIFFERENCE from the identity,
// D_l = I + (B - A) A^T (A A^T)^-1 with A = [Y_l(d_k)], B = [Y_l(R d_k)] - the same matrix as B A^+, but R = I gives B - A = 0 and
// with it D_l = I exactly.
bool band_matrices(const double* R, int deg, double* D) {
  double Al[N_DIR][25], Bl[N_DIR][25];
  for (int k = 0; k < N_DIR; ++k) {
    double d[3], e[3];
    sample_direction(k, d);
    for (int i = 0; i < 3; ++i) e[i] = R[3 * i] * d[0] + R[3 * i + 1] * d[1] + R[3 * i + 2] * d[2];
    sh_eval64(d[0], d[1], d[2], Al[k]);
    sh_eval64(e[0], e[1], e[2], Bl[k]);
  }
  for (int l = 1; l <= deg; ++l) {
    const int n = 2 * l + 1, o = l * l;
    double G[81], Gi[81], C[81];
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double g = 0., c = 0.;
        for (int k = 0; k < N_DIR; ++k) {
          g += Al[k][o + i] * Al[k][o + j];
          c += (Bl[k][o + i] - Al[k][o + i]) * Al[k][o + j];
        }
        G[i * n + j] = g;
        C[i * n + j] = c;
      }
    if (!invert(G, n, Gi)) return false;
    double* Dl = D + band_offset(l);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        double e = 0.;
        for (int k = 0; k < n; ++k) e += C[i * n + k] * Gi[k * n + j];
        Dl[i * n + j] = (i == j ? 1. : 0.) + e;
      }
  }
  return true;
}

// the unit quaternion (w, x, y, z), w >= 0, of an orthogonal R (Shepperd's branches: the largest of the four squares first)
void quat_of_rotation(const double* R, double* q) {
  const double m00 = R[0], m11 = R[4], m22 = R[8], tr = m00 + m11 + m22;
  if (tr > 0.) {
    const double s = 2. * std::sqrt(tr + 1.);
    q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
  } else if (m00 > m11 && m00 > m22) {
    const double s = 2. * std::sqrt(1. + m00 - m11 - m22);
    q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
  } else if (m11 > m22) {
    const double s = 2. * std::sqrt(1. + m11 - m00 - m22);
    q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
  } else {
    const double s = 2. * std::sqrt(1. + m22 - m00 - m11);
    q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
  }
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), sg = q[0] < 0. ? -1. : 1.;
  for (int i = 0; i < 4; ++i) q[i] = sg * q[i] / n;
}

// ---------------------------------------------------------------------------------------------------------------- transform

struct XformP {
  SplatView<const float> in;
  SplatView<float> out;
  float A[9], t[3], log_s, q[4];       // s R and t; log s; q_R as w x y z
  float D[N_COEF];
};

// the flat float e of the wave's harmonics is element c of row r: a lane's step of 64 floats is dq rows and dr columns
struct RowWalk {
  int r, c, dq, dr, W;
  __device__ RowWalk(int lane, int W_) : r(lane / W_), c(lane - (lane / W_) * W_), dq(WAVE / W_), dr(WAVE - (WAVE / W_) * W_), W(W_) {}
  __device__ void step() { c += dr; r += dq; if (c >= W) { c -= W; ++r; } }
};

// the harmonics rows of v follow each other without padding from a 16-byte boundary (and the LDS pitch is the row: ODD_ROW)
template <bool ODD_ROW, class T>
__device__ __forceinline__ bool flat_rows(const SplatView<T>& v, int W) {
  return ODD_ROW && v.ld[SPLAT_SH] == W && (((unsigned long long)(uintptr_t)v.p[SPLAT_SH]) & 15) == 0;
}

template <int DEG>
__global__ void __launch_bounds__(WAVE) splat_transform_kernel(const XformP a) {
  extern __shared__ __attribute__((aligned(16))) float s_sh[];      // [64][P]
  constexpr int NB = (DEG + 1) * (DEG + 1), W = 3 * NB, P = W | 1;
  const int lane = threadIdx.x;
  const long row0 = (long)blockIdx.x * WAVE, g = row0 + lane;
  const int nrow = (int)(a.in.rows - row0 < WAVE ? a.in.rows - row0 : WAVE);
  // Degrees 0, 2 and 4 have an odd row already (P == W): where the rows are contiguous and 16-byte aligned, the wave's harmonics
  // are one run of nrow W floats with the LDS image's own layout, moved 16 bytes per lane (64 row0 W floats: a multiple of 16 bytes)
  const int total = nrow * W;
  if (flat_rows<P == W>(a.in, W)) {
    const float* src = a.in.p[SPLAT_SH] + row0 * W;
    for (int i = lane; i < (total >> 2); i += WAVE) *(f32x4*)(s_sh + 4 * i) = *(const f32x4*)(src + 4 * i);
    for (int i = (total & ~3) + lane; i < total; i += WAVE) s_sh[i] = src[i];
  } else {
    RowWalk w(lane, W);
    for (int e = lane; e < total; e += WAVE) { s_sh[w.r * P + w.c] = a.in.sh(row0 + w.r)[w.c]; w.step(); }
  }
  const bool mine = lane < nrow;
  float m[3] = {0.f, 0.f, 0.f}, ls[3] = {0.f, 0.f, 0.f}, q[4] = {0.f, 0.f, 0.f, 0.f}, logit = 0.f;
  if (mine) {
#pragma unroll
    for (int e = 0; e < 3; ++e) { m[e] = a.in.means(g)[e]; ls[e] = a.in.ls(g)[e]; }
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = a.in.quats(g)[a.in.quat_slot(e)];     // w x y z
    logit = a.in.logit(g);
  }
  __syncthreads();     // every read of the wave's rows is done (in place: nothing of them has been written yet)
  if (mine) {
    float* row = s_sh + lane * P;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
#pragma unroll
      for (int l = 1; l <= DEG; ++l) {
        const int n = 2 * l + 1, o = ch * NB + l * l;
        const float* D = a.D + band_offset(l);
        float c[2 * MAX_DEG + 1], r[2 * MAX_DEG + 1];
#pragma unroll
        for (int j = 0; j < 2 * MAX_DEG + 1; ++j) c[j] = j < n ? row[o + j] : 0.f;
#pragma unroll
        for (int i = 0; i < 2 * MAX_DEG + 1; ++i) {
          if (i < n) {
            float acc = D[i * n] * c[0];
#pragma unroll
            for (int j = 1; j < 2 * MAX_DEG + 1; ++j) if (j < n) acc = fmaf(D[i * n + j], c[j], acc);
            r[i] = acc;
          }
        }
#pragma unroll
        for (int i = 0; i < 2 * MAX_DEG + 1; ++i) if (i < n) row[o + i] = r[i];
      }
    }
  }
  __syncthreads();
  if (mine) {
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      a.out.means(g)[e] = fmaf(a.A[3 * e], m[0], fmaf(a.A[3 * e + 1], m[1], fmaf(a.A[3 * e + 2], m[2], a.t[e])));
      a.out.ls(g)[e] = ls[e] + a.log_s;
    }
    const float rw = a.q[0], rx = a.q[1], ry = a.q[2], rz = a.q[3];
    float o[4];     // q_R (x) q, the Hamilton product
    o[0] = fmaf(-rz, q[3], fmaf(-ry, q[2], fmaf(-rx, q[1], rw * q[0])));
    o[1] = fmaf(-rz, q[2], fmaf(ry, q[3], fmaf(rx, q[0], rw * q[1])));
    o[2] = fmaf(rz, q[1], fmaf(ry, q[0], fmaf(-rx, q[3], rw * q[2])));
    o[3] = fmaf(rz, q[0], fmaf(-ry, q[1], fmaf(rx, q[2], rw * q[3])));
#pragma unroll
    for (int e = 0; e < 4; ++e) a.out.quats(g)[a.out.quat_slot(e)] = o[e];
    a.out.logit(g) = logit;
  }
  if (flat_rows<P == W>(a.out, W)) {
    float* dst = a.out.p[SPLAT_SH] + row0 * W;
    for (int i = lane; i < (total >> 2); i += WAVE) *(f32x4*)(dst + 4 * i) = *(const f32x4*)(s_sh + 4 * i);
    for (int i = (total & ~3) + lane; i < total; i += WAVE) dst[i] = s_sh[i];
  } else {
    RowWalk w(lane, W);
    for (int e = lane; e < total; e += WAVE) { a.out.sh(row0 + w.r)[w.c] = s_sh[w.r * P + w.c]; w.step(); }
  }
}

// the output tensors of the arguments under the field names splat_view_of reads
struct OutFields {
  float *means, *log_scales, *quats, *logits, *sh;
  long ld_means, ld_log_scales, ld_quats, ld_logits, ld_sh;
  int quats_xyzw;
};

int degree_of(int K) {     // K + 1 = (deg + 1)^2, or -1
  for (int d = 0; d <= MAX_DEG; ++d)
    if (K + 1 == (d + 1) * (d + 1)) return d;
  return -1;
}

// ------------------------------------------------------------------------------------------------------------------ moments

struct MomP {
  const float* means; long ld, n;
  double c[3];
  double* part; long tiles;       // [tiles][10]
  double* out;
};

// The ten sums of a tile of 1024 rows: a lane adds the rows tile + j 256 + lane, j = 0..3, in this order, then block_sum
__global__ void __launch_bounds__(MOM_THREADS) splat_moments_kernel(const MomP a) {
  __shared__ double red[MOM_THREADS];
  double s[MOM_OUT];
#pragma unroll
  for (int k = 0; k < MOM_OUT; ++k) s[k] = 0.;
  const long first = (long)blockIdx.x * MOM_TILE;
#pragma unroll
  for (int j = 0; j < MOM_ITEMS; ++j) {
    const long r = first + j * MOM_THREADS + threadIdx.x;
    if (r < a.n) {
      const float* p = a.means + r * a.ld;
      const double x = (double)p[0] - a.c[0], y = (double)p[1] - a.c[1], z = (double)p[2] - a.c[2];
      s[0] += 1.; s[1] += x; s[2] += y; s[3] += z;
      s[4] += x * x; s[5] += x * y; s[6] += x * z; s[7] += y * y; s[8] += y * z; s[9] += z * z;
    }
  }
#pragma unroll
  for (int k = 0; k < MOM_OUT; ++k) {
    const double tot = block_sum<MOM_THREADS>(s[k], red);
    if (threadIdx.x == 0) a.part[(long)blockIdx.x * MOM_OUT + k] = tot;
  }
}

// one workgroup: each lane adds the partials tid, tid + 256, ... in index order, then block_sum
__global__ void __launch_bounds__(MOM_THREADS) splat_moments_reduce_kernel(const MomP a) {
  __shared__ double red[MOM_THREADS];
#pragma unroll
  for (int k = 0; k < MOM_OUT; ++k) {
    double s = 0.;
    for (long i = threadIdx.x; i < a.tiles; i += MOM_THREADS) s += a.part[i * MOM_OUT + k];
    const double tot = block_sum<MOM_THREADS>(s, red);
    if (threadIdx.x == 0) a.out[k] = tot;
  }
}

}  // namespace

extern "C" int v3a_sh_rotation_matrices(const double* R, int deg, double* out) {
  if (!R || (deg > 0 && !out)) return V3A_ERR_ARG;
  if (deg < 0 || deg > MAX_DEG) return V3A_ERR_SHAPE;
  if (check_rotation(R) != V3A_OK) return V3A_ERR_ARG;
  double P[9], D[N_COEF];
  polish_rotation(R, P);
  if (!band_matrices(P, deg, D)) return V3A_ERR_ARG;
  for (int i = 0; i < band_offset(deg + 1); ++i) out[i] = D[i];
  return V3A_OK;
}

extern "C" int v3a_splat_transform(const v3a_splat_transform_args* a, void* stream) {
  XformP k{};
  int rc = splat_view_of(a, a ? a->rows : 0, a ? a->K : 0, k.in);
  if (rc != V3A_OK) return rc;
  const int deg = degree_of(a->K);
  if (deg < 0) return V3A_ERR_SHAPE;
  if (!(a->scale > 0.) || !std::isfinite(a->scale) || check_rotation(a->R) != V3A_OK) return V3A_ERR_ARG;
  for (int e = 0; e < 3; ++e)
    if (!std::isfinite(a->t[e])) return V3A_ERR_ARG;
  if (a->rows == 0) return V3A_OK;
  const OutFields o{a->out_means, a->out_log_scales, a->out_quats, a->out_logits, a->out_sh,
                    a->out_ld_means, a->out_ld_log_scales, a->out_ld_quats, a->out_ld_logits, a->out_ld_sh, a->quats_xyzw};
  if ((rc = splat_view_of(&o, a->rows, a->K, k.out)) != V3A_OK) return rc;
  double P[9], q[4], D[N_COEF] = {0.};
  polish_rotation(a->R, P);
  if (!band_matrices(P, deg, D)) return V3A_ERR_ARG;
  quat_of_rotation(P, q);
  for (int e = 0; e < 9; ++e) k.A[e] = (float)(a->scale * a->R[e]);
  for (int e = 0; e < 3; ++e) k.t[e] = (float)a->t[e];
  k.log_s = (float)std::log(a->scale);
  for (int e = 0; e < 4; ++e) k.q[e] = (float)q[e];
  for (int e = 0; e < N_COEF; ++e) k.D[e] = (float)D[e];
  const dim3 grid((unsigned)blocks_for(a->rows, WAVE)), block(WAVE);
  const size_t lds = (size_t)WAVE * ((3 * (a->K + 1)) | 1) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  switch (deg) {
    case 0: hipLaunchKernelGGL(splat_transform_kernel<0>, grid, block, lds, s, k); break;
    case 1: hipLaunchKernelGGL(splat_transform_kernel<1>, grid, block, lds, s, k); break;
    case 2: hipLaunchKernelGGL(splat_transform_kernel<2>, grid, block, lds, s, k); break;
    case 3: hipLaunchKernelGGL(splat_transform_kernel<3>, grid, block, lds, s, k); break;
    default: hipLaunchKernelGGL(splat_transform_kernel<4>, grid, block, lds, s, k); break;
  }
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" long v3a_splat_moments_workspace_bytes(long n) {
  if (bad_count(n)) return V3A_ERR_SHAPE;
  return (long)align256((size_t)blocks_for(n, MOM_TILE) * MOM_OUT * sizeof(double));
}

extern "C" int v3a_splat_moments(const float* means, long ld_means, long n, const double* centre, double* out, void* workspace,
                                 long workspace_bytes, void* stream) {
  if (bad_count(n)) return V3A_ERR_SHAPE;
  if (!centre || !out || (n > 0 && !means)) return V3A_ERR_ARG;
  if (n > 0 && ld_means < 3) return V3A_ERR_SHAPE;
  for (int e = 0; e < 3; ++e)
    if (!std::isfinite(centre[e])) return V3A_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return hipMemsetAsync(out, 0, MOM_OUT * sizeof(double), s) == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
  if (bad_workspace(workspace, workspace_bytes, v3a_splat_moments_workspace_bytes(n))) return V3A_ERR_WORKSPACE;
  MomP k{means, ld_means, n, {centre[0], centre[1], centre[2]}, (double*)workspace, blocks_for(n, MOM_TILE), out};
  hipLaunchKernelGGL(splat_moments_kernel, dim3((unsigned)k.tiles), dim3(MOM_THREADS), 0, s, k);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(splat_moments_reduce_kernel, dim3(1), dim3(MOM_THREADS), 0, s, k);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
