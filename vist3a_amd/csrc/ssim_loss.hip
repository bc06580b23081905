// Photometric loss of the post-optimisation loop, forward and backward:
//   loss = (1 - lambda) * l1 + lambda * (1 - ssim),   l1 = mean |pred - target|,   ssim = mean SSIM map
// on fp32 [N,H,W,C] images (C <= 4), the layout the rasteriser emits.  Replaces, for
// third_party_model/anysplat/src/post_opt/simple_trainer.py:938-942, F.l1_loss + fused_ssim(padding="valid").
//
// SSIM is the reference's loss/loss_ssim.py::ssim(X, Y, data_range=1.0, size_average=True): 11-tap Gaussian (sigma 1.5), separable
// *valid* filtering of x, y, x^2, y^2, xy, population variances, C1 = 1e-4, C2 = 9e-4, mean over the (H-10) x (W-10) map, all
// channels and images.  The reference builds its taps in float32 (exp and the division by the sum) and casts them to the working
// dtype; TAPS below are those eleven float32 values, so that this file and the reference filter with the same numbers.
//
// Arithmetic: the inputs are fp32, everything after the load is fp64 (the map, the three derivative planes, the partial sums).  The
// variances are differences of nearly equal moments; in fp32 the reference itself loses 4e-6 of the value and 7e-5 of the gradient
// on smooth images (tests/golden/make_golden_ssim_loss.py prints both).  At 448 x 448 x 3 the pass is launch-bound either way.
//
// No border logic: a map position's window never reads past an edge.  Forward: one workgroup = one 16 x 32 tile of map positions of
// one channel of one image; it stages the tile + 10 rows / columns of both images in LDS, runs the vertical pass of the five
// moments into LDS, then the horizontal pass, S and its derivatives in registers, and writes one fp64 partial of S, one of |x - y|
// (tiles next to an image edge own the border pixels, as in image_metrics.hip) and, when the caller asks for a gradient, the three
// planes dS/dmu1 (total), dS/dE[x^2], dS/dE[xy] of its positions.  A second launch (one workgroup) adds the partials in the order of
// fixed_sum.h and writes loss, l1, ssim.  Backward, gather form: one workgroup = one 16 x 32 tile of INPUT pixels; pixel p sums over the
// at most 11 x 11 map positions q whose window covers it  w(p - q) (dmu1(q) + 2 x(p) dxx(q) + y(p) dxy(q)),  separably (vertical
// pass of the three planes into LDS, horizontal pass in registers), adds the L1 term and writes d_pred once.  No atomics anywhere:
// bit-identical run to run, and exactly linear in the incoming gradient.
#include "common.h"
#include "fixed_sum.h"
#include "../../include/vist3a_hip.h"

// No contraction in this file: identical images must give 2 mu1 mu2 + C1 == mu1^2 + mu2^2 + C1 (and the variance pair) bit for
// bit, so that ssim == 1, l1 == 0 and loss == 0 exactly.
#pragma clang fp contract(off)

namespace {

constexpr int TH = 16, TW = 32;        // tile: map positions (forward) / input pixels (backward)
constexpr int RAD2 = 10;               // window size - 1
constexpr int NT = RAD2 + 1;
constexpr int RH = TH + RAD2, RW = TW + RAD2;   // staged rows / columns (26 x 42)
constexpr int PITCH = RW + 1;
constexpr int MAXC = 4;
constexpr int THREADS = 256;

// float32(exp(-(k - 5)^2 / 4.5) / sum), as torch computes them in loss_ssim.py::_fspecial_gauss_1d
__constant__ const double TAPS[NT] = {0x1.0d957p-10, 0x1.f1fe02p-8, 0x1.26eb18p-5, 0x1.bff0fep-4, 0x1.b43c3ep-3, 0x1.10656p-2,
                                      0x1.b43c3ep-3, 0x1.bff0fep-4, 0x1.26eb18p-5, 0x1.f1fe02p-8, 0x1.0d957p-10};

struct LossP {
  const float* x;      // pred
  const float* y;      // target
  double* part_s;      // [N][C][tiles]
  double* part_l;      // [N][C][tiles]
  double* planes;      // [3][N][C][Hm][Wm] or null
  int N, H, W, C, Hm, Wm, tiles_x, tiles_y;
};

__global__ void __launch_bounds__(THREADS) ssim_loss_fwd_kernel(LossP p) {
  __shared__ float pl[2][RH][PITCH];
  __shared__ double vm[5][TH][PITCH];   // vertical-pass moments: tile rows x staged columns
  __shared__ double red[THREADS];

  const int tid = threadIdx.x;
  const int tile = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int ty = tile / p.tiles_x, tx = tile % p.tiles_x;
  const int H = p.H, W = p.W, C = p.C;
  const int qy0 = ty * TH, qx0 = tx * TW;                         // first map position of the tile = first staged input pixel
  const int th = min(TH, p.Hm - qy0), tw = min(TW, p.Wm - qx0);
  const int rh = th + RAD2, rw = tw + RAD2;                       // staged region: rows qy0 .. qy0 + th + 9 < H

  // 1. stage this channel of both images; |x - y| of the owned pixels (the tile's first th x tw pixels, and the 10-pixel border
  //    at the image's bottom / right edge for the last tile row / column: every pixel is counted exactly once)
  const size_t img = (size_t)n * H * W * C;
  const int own_h = ty == p.tiles_y - 1 ? rh : th, own_w = tx == p.tiles_x - 1 ? rw : tw;
  double l1 = 0.0;
  for (int i = tid; i < rh * rw; i += THREADS) {
    const int r = i / rw, k = i % rw;
    const size_t o = img + ((size_t)(qy0 + r) * W + (qx0 + k)) * C + c;
    const float a = p.x[o], b = p.y[o];
    pl[0][r][k] = a;
    pl[1][r][k] = b;
    if (r < own_h && k < own_w) l1 += fabs((double)a - (double)b);
  }
  __syncthreads();

  // 2. vertical pass of the five moments at the tile's rows, every staged column
  for (int i = tid; i < th * rw; i += THREADS) {
    const int r = i / rw, k = i % rw;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const double a = (double)pl[0][r + j][k], b = (double)pl[1][r + j][k], w = TAPS[j];
      sx += w * a;
      sy += w * b;
      sxx += w * (a * a);
      syy += w * (b * b);
      sxy += w * (a * b);
    }
    vm[0][r][k] = sx;
    vm[1][r][k] = sy;
    vm[2][r][k] = sxx;
    vm[3][r][k] = syy;
    vm[4][r][k] = sxy;
  }
  __syncthreads();

  // 3. horizontal pass, S and its derivatives
  const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
  const size_t plane = (size_t)p.N * C * p.Hm * p.Wm;
  double ssum = 0.0;
  for (int i = tid; i < th * TW; i += THREADS) {
    const int r = i / TW, k = i % TW;
    if (k >= tw) continue;
    double u[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < NT; ++j) acc += TAPS[j] * vm[m][r][k + j];
      u[m] = acc;
    }
    const double mu1 = u[0], mu2 = u[1];
    const double mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
    const double s1 = u[2] - mu1_sq, s2 = u[3] - mu2_sq, s12 = u[4] - mu12;
    const double A1 = 2.0 * mu12 + C1, B1 = mu1_sq + mu2_sq + C1, A2 = 2.0 * s12 + C2, B2 = s1 + s2 + C2;
    const double lum = A1 / B1, cs = A2 / B2;
    const double S = lum * cs;
    ssum += S;
    if (p.planes) {
      const double dxx = -S / B2;               // dS / dE[x^2]  (= dS / dsigma1^2)
      const double dxy = 2.0 * lum / B2;        // dS / dE[xy]   (= dS / dsigma12)
      const double dmu = cs * (2.0 * mu2 / B1 - 2.0 * mu1 * lum / B1) - 2.0 * mu1 * dxx - mu2 * dxy;   // total dS / dmu1
      const size_t o = (((size_t)n * C + c) * p.Hm + (qy0 + r)) * p.Wm + (qx0 + k);
      p.planes[o] = dmu;
      p.planes[plane + o] = dxx;
      p.planes[2 * plane + o] = dxy;
    }
  }

  const double ts = block_sum<THREADS>(ssum, red);
  const double tl = block_sum<THREADS>(l1, red);
  if (tid == 0) {
    const size_t o = ((size_t)n * C + c) * (p.tiles_x * p.tiles_y) + tile;
    p.part_s[o] = ts;
    p.part_l[o] = tl;
  }
}

// out[0] = loss, out[1] = l1, out[2] = ssim.  One workgroup, partials in index order per lane, then the fixed tree.
__global__ void __launch_bounds__(THREADS) ssim_loss_reduce_kernel(const double* part_s, const double* part_l, long parts, double count,
                                                                    double numel, double lambda, double* out) {
  __shared__ double red[THREADS];
  const int tid = threadIdx.x;
  double ps = 0.0, pl = 0.0;
  for (long t = tid; t < parts; t += THREADS) {
    ps += part_s[t];
    pl += part_l[t];
  }
  const double s = block_sum<THREADS>(ps, red), l = block_sum<THREADS>(pl, red);
  if (tid == 0) {
    const double ssim = s / count, l1 = l / numel;   // divisions: a sum of `count` ones gives exactly 1
    out[0] = (1.0 - lambda) * l1 + lambda * (1.0 - ssim);
    out[1] = l1;
    out[2] = ssim;
  }
}

struct LossBwdP {
  const float* x;
  const float* y;
  const double* planes;
  const double* d_out;   // [3]: gradients of loss, l1, ssim
  float* d_x;
  int N, H, W, C, Hm, Wm, tiles_x;
  double lambda, inv_count, inv_numel;
};

__global__ void __launch_bounds__(THREADS) ssim_loss_bwd_kernel(LossBwdP p) {
  __shared__ double pq[3][RH][PITCH];   // planes at map rows py0 - 10 .. py0 + th - 1, columns px0 - 10 .. px0 + tw - 1 (zero outside the map)
  __shared__ double vq[3][TH][PITCH];

  const int tid = threadIdx.x;
  const int tile = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int ty = tile / p.tiles_x, tx = tile % p.tiles_x;
  const int H = p.H, W = p.W, C = p.C;
  const int py0 = ty * TH, px0 = tx * TW;
  const int th = min(TH, H - py0), tw = min(TW, W - px0);
  const int rh = th + RAD2, rw = tw + RAD2;
  const size_t plane = (size_t)p.N * C * p.Hm * p.Wm;
  const size_t pbase = ((size_t)n * C + c) * p.Hm * p.Wm;

  for (int i = tid; i < rh * rw; i += THREADS) {
    const int r = i / rw, k = i % rw;
    const int qy = py0 - RAD2 + r, qx = px0 - RAD2 + k;
    const bool in = qy >= 0 && qy < p.Hm && qx >= 0 && qx < p.Wm;
    const size_t o = pbase + (size_t)(in ? qy : 0) * p.Wm + (in ? qx : 0);
#pragma unroll
    for (int m = 0; m < 3; ++m) pq[m][r][k] = in ? p.planes[m * plane + o] : 0.0;
  }
  __syncthreads();

  // vertical: pixel row py0 + r takes map rows py - j, j = 0..10, i.e. staged rows r + 10 - j, with tap j
  for (int i = tid; i < th * rw; i += THREADS) {
    const int r = i / rw, k = i % rw;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const double w = TAPS[j];
      a0 += w * pq[0][r + RAD2 - j][k];
      a1 += w * pq[1][r + RAD2 - j][k];
      a2 += w * pq[2][r + RAD2 - j][k];
    }
    vq[0][r][k] = a0;
    vq[1][r][k] = a1;
    vq[2][r][k] = a2;
  }
  __syncthreads();

  const double g_loss = p.d_out[0], g_l1 = p.d_out[1], g_ssim = p.d_out[2];
  const double gl = ((1.0 - p.lambda) * g_loss + g_l1) * p.inv_numel;
  const double gs = (g_ssim - p.lambda * g_loss) * p.inv_count;
  const size_t img = (size_t)n * H * W * C;
  for (int i = tid; i < th * TW; i += THREADS) {
    const int r = i / TW, k = i % TW;
    if (k >= tw) continue;
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const double w = TAPS[j];
      g0 += w * vq[0][r][k + RAD2 - j];
      g1 += w * vq[1][r][k + RAD2 - j];
      g2 += w * vq[2][r][k + RAD2 - j];
    }
    const size_t o = img + ((size_t)(py0 + r) * W + (px0 + k)) * C + c;
    const double a = (double)p.x[o], b = (double)p.y[o];
    const double sg = a > b ? 1.0 : (a < b ? -1.0 : 0.0);
    p.d_x[o] = (float)(gl * sg + gs * (g0 + 2.0 * a * g1 + b * g2));
  }
}

bool bad_shape(int N, int H, int W, int C) {
  return N < 1 || N > 65535 || C < 1 || C > MAXC || H < NT || W < NT;
}

long fwd_tiles(int H, int W) {
  return (long)((H - RAD2 + TH - 1) / TH) * ((W - RAD2 + TW - 1) / TW);
}

}  // namespace

extern "C" long v3a_photometric_loss_workspace_bytes(int N, int H, int W, int C) {
  if (bad_shape(N, H, W, C)) return V3A_ERR_SHAPE;
  return 2L * N * C * fwd_tiles(H, W) * (long)sizeof(double);
}

extern "C" long v3a_photometric_loss_planes_bytes(int N, int H, int W, int C) {
  if (bad_shape(N, H, W, C)) return V3A_ERR_SHAPE;
  return 3L * N * C * (H - RAD2) * (W - RAD2) * (long)sizeof(double);
}

extern "C" int v3a_photometric_loss_forward(const v3a_photometric_loss_args* a, void* stream) {
  if (!a || !a->pred || !a->target || !a->out) return V3A_ERR_ARG;
  if (bad_shape(a->N, a->H, a->W, a->C)) return V3A_ERR_SHAPE;
  if (!a->workspace || a->workspace_bytes < v3a_photometric_loss_workspace_bytes(a->N, a->H, a->W, a->C)) return V3A_ERR_WORKSPACE;
  if (a->planes && a->planes_bytes < v3a_photometric_loss_planes_bytes(a->N, a->H, a->W, a->C)) return V3A_ERR_WORKSPACE;
  LossP p;
  p.x = a->pred;
  p.y = a->target;
  p.N = a->N; p.H = a->H; p.W = a->W; p.C = a->C;
  p.Hm = a->H - RAD2;
  p.Wm = a->W - RAD2;
  p.tiles_x = (p.Wm + TW - 1) / TW;
  p.tiles_y = (p.Hm + TH - 1) / TH;
  const long parts = (long)a->N * a->C * p.tiles_x * p.tiles_y;
  p.part_s = (double*)a->workspace;
  p.part_l = p.part_s + parts;
  p.planes = a->planes;
  hipLaunchKernelGGL(ssim_loss_fwd_kernel, dim3(p.tiles_x * p.tiles_y, a->C, a->N), dim3(THREADS), 0, (hipStream_t)stream, p);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  const double count = (double)a->N * a->C * p.Hm * p.Wm, numel = (double)a->N * a->C * a->H * a->W;
  hipLaunchKernelGGL(ssim_loss_reduce_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, p.part_s, p.part_l, parts, count, numel,
                     (double)a->ssim_lambda, a->out);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_photometric_loss_backward(const v3a_photometric_loss_args* a, const double* d_out, float* d_pred, void* stream) {
  if (!a || !a->pred || !a->target || !a->planes || !d_out || !d_pred) return V3A_ERR_ARG;
  if (bad_shape(a->N, a->H, a->W, a->C)) return V3A_ERR_SHAPE;
  if (a->planes_bytes < v3a_photometric_loss_planes_bytes(a->N, a->H, a->W, a->C)) return V3A_ERR_WORKSPACE;
  LossBwdP p;
  p.x = a->pred;
  p.y = a->target;
  p.planes = a->planes;
  p.d_out = d_out;
  p.d_x = d_pred;
  p.N = a->N; p.H = a->H; p.W = a->W; p.C = a->C;
  p.Hm = a->H - RAD2;
  p.Wm = a->W - RAD2;
  p.tiles_x = (a->W + TW - 1) / TW;
  const int tiles_y = (a->H + TH - 1) / TH;
  p.lambda = (double)a->ssim_lambda;
  p.inv_count = 1.0 / ((double)a->N * a->C * p.Hm * p.Wm);
  p.inv_numel = 1.0 / ((double)a->N * a->C * a->H * a->W);
  hipLaunchKernelGGL(ssim_loss_bwd_kernel, dim3(p.tiles_x * tiles_y, a->C, a->N), dim3(THREADS), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
