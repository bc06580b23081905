// Image-pair quality metrics of the novel-view-synthesis evaluation: SSIM and MSE (-> PSNR on the host) of uint8 image pairs.
//
// Replaces, for the RE10K protocol of evaluation/novel_view_synthesis_bench/calculate_metric.py, the reference's per-image host calls
// third_party_model/anysplat/src/evaluation/metrics.py:11-19 (compute_psnr) and :44-55 (skimage structural_similarity with
// win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0).  Pixels are uint8 / 255 in fp32, what ToTensor makes of the
// PNGs the reference re-reads from disk.
//
// SSIM, as skimage computes it: the five moment planes ux, uy, E[x^2], E[y^2], E[xy] are filtered separably with the 11-tap
// Gaussian (sigma 1.5, truncate 3.5; taps exp(-x^2 / 2 sigma^2) / sum, computed by the host in double and applied in double
// like scipy's correlate1d, each pass rounded to float32), variances and covariance
// are scaled by cov_norm = 121/120 (sample covariance), C1 = 0.01^2, C2 = 0.03^2, and S is averaged over the interior crop
// [5, H-5) x [5, W-5) of each channel, then over the channels.
//
// No border logic: every kept output pixel lies at least 5 pixels inside the image, so its 11x11 window never reads past an
// edge.  The `reflect` padding of scipy's gaussian_filter only ever feeds output pixels that the crop throws away, so this kernel
// tiles the crop alone and reads only real pixels.
//
// Shape: one workgroup = one 32x32 tile of kept outputs of one channel of one pair.  It stages the tile + 5-pixel halo of both
// images in LDS (dword loads of the interleaved NHWC rows), converts its channel to fp32 planes, runs the horizontal pass
// (scipy's order: the vertical pass first, 5 moments, into LDS), then the horizontal pass and S in registers, and writes one fp64 partial sum of S and one of the
// squared error.  A second launch reduces each pair's partials in the order of fixed_sum.h: no float atomics, bit-identical run to run.
// MSE ownership: the tile rows / columns next to an image edge also own the 5-pixel border, so every pixel of every channel is
// counted exactly once (halo pixels are counted by the tile that owns them).
#include "common.h"
#include "fixed_sum.h"
#include "../../include/vist3a_hip.h"

// No contraction in this file: with fused multiply-adds, 2 ux uy + C1 and ux^2 + uy^2 + C1 (and the variance pair) could round
// differently for identical images, whose SSIM must come out exactly 1.
#pragma clang fp contract(off)

namespace {

constexpr int TILE = 32;               // kept outputs per tile side
constexpr int RAD = 5;                 // (win_size - 1) / 2
constexpr int TAPS = 2 * RAD + 1;
constexpr int RD = TILE + 2 * RAD;     // staged rows / columns (42)
constexpr int MAXC = 4;
constexpr int RAW_PITCH = (RD * MAXC + 3 + 3) / 4;   // dwords per staged byte row (43: a row of <= 168 bytes + 3 alignment bytes)
constexpr int PL_PITCH = RD + 1;
constexpr int THREADS = 256;

struct Taps {
  double w[RAD + 1];   // centre tap, then offsets 1..5 (symmetric)
};

struct MetricsP {
  const unsigned char* a;
  const unsigned char* b;
  double* part_s;     // [N][C][tiles]
  double* part_e;     // [N][C][tiles]
  int H, W, C, tiles_x, tiles;
};

__global__ void __launch_bounds__(THREADS) ssim_tile_kernel(MetricsP p, Taps tp) {
  __shared__ unsigned int raw[2][RD][RAW_PITCH];
  __shared__ float pl[2][RD][PL_PITCH];
  __shared__ float hm[5][TILE][PL_PITCH];   // vertical-pass moments: kept rows x staged columns
  __shared__ double red[THREADS];

  const int tid = threadIdx.x;
  const int tile = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int ty = tile / p.tiles_x, tx = tile % p.tiles_x;
  const int H = p.H, W = p.W, C = p.C;
  const int oy0 = RAD + ty * TILE, ox0 = RAD + tx * TILE;          // first kept output of the tile
  const int th = min(TILE, H - RAD - oy0), tw = min(TILE, W - RAD - ox0);
  const int rh = th + 2 * RAD, rw = tw + 2 * RAD;                  // staged region: rows oy0-5 .. oy0+th+4 (all inside the image)
  const int y0 = oy0 - RAD, x0 = ox0 - RAD;

  // 1. stage both images' region rows, all channels, as aligned dwords (bytes outside the row segment are never read)
  const size_t img = (size_t)n * H * W * C;
  const int rowb = rw * C;
  for (int i = tid; i < 2 * rh * RAW_PITCH; i += THREADS) {
    const int k = i % RAW_PITCH, r = (i / RAW_PITCH) % rh, im = i / (RAW_PITCH * rh);
    const unsigned char* base = (im ? p.b : p.a) + img + ((size_t)(y0 + r) * W + x0) * C;
    const uintptr_t s = (uintptr_t)base, e = s + rowb, q = (s & ~(uintptr_t)3) + 4 * (uintptr_t)k;
    unsigned int v = 0;
    if (q >= s && q + 4 <= e) {
      v = *(const unsigned int*)q;
    } else if (q < e) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (q + j >= s && q + j < e) v |= (unsigned int)(*(const unsigned char*)(q + j)) << (8 * j);
    }
    raw[im][r][k] = v;
  }
  __syncthreads();

  // 2. this channel as fp32 planes (ToTensor: u8 / 255); squared error of the owned pixels
  const int rlo = ty == 0 ? 0 : RAD, rhi = ty == p.tiles / p.tiles_x - 1 ? rh : RAD + th;
  const int clo = tx == 0 ? 0 : RAD, chi = tx == p.tiles_x - 1 ? rw : RAD + tw;
  double err = 0.0;
  for (int i = tid; i < rh * rw; i += THREADS) {
    const int r = i / rw, x = i % rw;
    // the row start's alignment is the same for every row only when W * C % 4 == 0: take it per row
    const int oa = (int)((uintptr_t)(p.a + img + ((size_t)(y0 + r) * W + x0) * C) & 3);
    const int ob = (int)((uintptr_t)(p.b + img + ((size_t)(y0 + r) * W + x0) * C) & 3);
    const int ba = oa + x * C + c, bb = ob + x * C + c;
    const float va = (float)((raw[0][r][ba >> 2] >> (8 * (ba & 3))) & 0xffu) / 255.0f;
    const float vb = (float)((raw[1][r][bb >> 2] >> (8 * (bb & 3))) & 0xffu) / 255.0f;
    pl[0][r][x] = va;
    pl[1][r][x] = vb;
    if (r >= rlo && r < rhi && x >= clo && x < chi) {
      const float d = va - vb;
      err += (double)(d * d);
    }
  }
  __syncthreads();

  // 3. vertical pass (scipy filters axis 0 first) at the tile's kept rows, every staged column.  Each 1-D pass is scipy's
  // correlate1d with symmetric weights: double accumulation w0 x0 + sum_{j=5..1} (x-j + x+j) wj, rounded to float32 on store -
  // the moment planes come out as skimage's float32 arrays.
  for (int i = tid; i < th * rw; i += THREADS) {
    const int r = i / rw, x = i % rw;
    const float a0 = pl[0][r + RAD][x], b0 = pl[1][r + RAD][x];
    double sx = (double)a0 * tp.w[0], sy = (double)b0 * tp.w[0], sxx = (double)(a0 * a0) * tp.w[0], syy = (double)(b0 * b0) * tp.w[0],
           sxy = (double)(a0 * b0) * tp.w[0];
#pragma unroll
    for (int j = RAD; j >= 1; --j) {
      const float al = pl[0][r + RAD - j][x], ar = pl[0][r + RAD + j][x], bl = pl[1][r + RAD - j][x], br = pl[1][r + RAD + j][x];
      const double w = tp.w[j];
      sx += ((double)al + (double)ar) * w;
      sy += ((double)bl + (double)br) * w;
      sxx += ((double)(al * al) + (double)(ar * ar)) * w;
      syy += ((double)(bl * bl) + (double)(br * br)) * w;
      sxy += ((double)(al * bl) + (double)(ar * br)) * w;
    }
    hm[0][r][x] = (float)sx;
    hm[1][r][x] = (float)sy;
    hm[2][r][x] = (float)sxx;
    hm[3][r][x] = (float)syy;
    hm[4][r][x] = (float)sxy;
  }
  __syncthreads();

  // 4. horizontal pass + S in float32 with numpy's operation order (skimage structural_similarity)
  double ssum = 0.0;
  for (int i = tid; i < th * TILE; i += THREADS) {
    const int r = i / TILE, j = i % TILE;
    if (j >= tw) continue;
    float u[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) {
      double acc = (double)hm[m][r][j + RAD] * tp.w[0];
#pragma unroll
      for (int k = RAD; k >= 1; --k) acc += ((double)hm[m][r][j + RAD - k] + (double)hm[m][r][j + RAD + k]) * tp.w[k];
      u[m] = (float)acc;
    }
    const float ux = u[0], uy = u[1], uxx = u[2], uyy = u[3], uxy = u[4];
    {
      const float cov_norm = (float)(121.0 / 120.0), C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);   // numpy: float32(python float)
      const float vx = cov_norm * (uxx - ux * ux);
      const float vy = cov_norm * (uyy - uy * uy);
      const float vxy = cov_norm * (uxy - ux * uy);
      const float A1 = 2.0f * ux * uy + C1, A2 = 2.0f * vxy + C2;
      const float B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
      const float num = A1 * A2, den = B1 * B2;
      // float32 S correctly rounded (the double quotient rounds to the same float); num / num is exactly 1
      ssum += (double)(float)((double)num / (double)den);
    }
  }

  const double ts = block_sum<THREADS>(ssum, red);
  const double te = block_sum<THREADS>(err, red);
  if (tid == 0) {
    const size_t o = ((size_t)n * C + c) * p.tiles + tile;
    p.part_s[o] = ts;
    p.part_e[o] = te;
  }
}

__global__ void __launch_bounds__(THREADS) metrics_reduce_kernel(const double* part_s, const double* part_e, int C, int tiles,
                                                                  double inv_count, double inv_pixels, double* ssim, double* mse) {
  __shared__ double red[THREADS];
  const int n = blockIdx.x, tid = threadIdx.x;
  double s_acc = 0.0, e_acc = 0.0;
  for (int c = 0; c < C; ++c) {
    const size_t o = ((size_t)n * C + c) * tiles;
    double ps = 0.0, pe = 0.0;
    for (int t = tid; t < tiles; t += THREADS) {
      ps += part_s[o + t];
      pe += part_e[o + t];
    }
    s_acc += block_sum<THREADS>(ps, red) * inv_count;     // this channel's mean S over the crop
    e_acc += block_sum<THREADS>(pe, red);
  }
  if (tid == 0) {
    ssim[n] = s_acc / C;
    mse[n] = e_acc * inv_pixels;
  }
}

int tiles_of(int H, int W, int* tiles_x) {
  const int tx = (W - 2 * RAD + TILE - 1) / TILE, ty = (H - 2 * RAD + TILE - 1) / TILE;
  if (tiles_x) *tiles_x = tx;
  return tx * ty;
}

bool bad_shape(int N, int H, int W, int C) {
  return N < 1 || C < 1 || C > MAXC || H < TAPS || W < TAPS;
}

}  // namespace

extern "C" long v3a_image_metrics_workspace_bytes(int N, int H, int W, int C) {
  if (bad_shape(N, H, W, C)) return V3A_ERR_SHAPE;
  return 2L * N * C * tiles_of(H, W, nullptr) * (long)sizeof(double);
}

extern "C" int v3a_image_metrics(const v3a_image_metrics_args* a, void* stream) {
  if (!a || !a->a || !a->b || !a->ssim || !a->mse) return V3A_ERR_ARG;
  if (bad_shape(a->N, a->H, a->W, a->C)) return V3A_ERR_SHAPE;
  const long need = v3a_image_metrics_workspace_bytes(a->N, a->H, a->W, a->C);
  if (!a->workspace || a->workspace_bytes < need) return V3A_ERR_WORKSPACE;

  MetricsP p;
  p.a = (const unsigned char*)a->a;
  p.b = (const unsigned char*)a->b;
  p.H = a->H;
  p.W = a->W;
  p.C = a->C;
  p.tiles = tiles_of(a->H, a->W, &p.tiles_x);
  const size_t parts = (size_t)a->N * a->C * p.tiles;
  p.part_s = (double*)a->workspace;
  p.part_e = p.part_s + parts;
  // scipy.ndimage._gaussian_kernel1d(1.5, 0, 5): exp(-x^2 / (2 sigma^2)) normalised by its sum, in double
  Taps tp;
  double phi[TAPS];
  for (int k = 0; k < TAPS; ++k) phi[k] = exp(-0.5 / (1.5 * 1.5) * (double)((k - RAD) * (k - RAD)));
  // numpy's sum of 11 values: eight partial sums combined pairwise, then the remaining three in order
  double sum = ((phi[0] + phi[1]) + (phi[2] + phi[3])) + ((phi[4] + phi[5]) + (phi[6] + phi[7]));
  for (int k = 8; k < TAPS; ++k) sum += phi[k];
  for (int k = 0; k <= RAD; ++k) tp.w[k] = phi[RAD + k] / sum;

  hipLaunchKernelGGL(ssim_tile_kernel, dim3(p.tiles, a->C, a->N), dim3(THREADS), 0, (hipStream_t)stream, p, tp);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  const double count = (double)(a->H - 2 * RAD) * (a->W - 2 * RAD), pixels = (double)a->H * a->W * a->C;
  hipLaunchKernelGGL(metrics_reduce_kernel, dim3(a->N), dim3(THREADS), 0, (hipStream_t)stream, p.part_s, p.part_e, a->C, p.tiles,
                     1.0 / count, 1.0 / pixels, a->ssim, a->mse);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
