// Depth term of the post-optimisation loop, forward and backward: an L1 in disparity space between the rasteriser's EXPECTED depth
// and a dense target map, third_party_model/anysplat/src/post_opt/simple_trainer.py:943-961 with `points` = the integer pixel
// coordinates of the used pixels (grid_sample(align_corners=True) at an integer pixel returns that pixel).
//
// Inputs: depth, alpha f32 [C,H,W] as v3a_gs_rasterize emits them (depth = the alpha-weighted z, gsplat's "RGB+D"), depth_gt f32
// [C,H,W], mask uint8 [C,H,W] (nonzero = use the pixel; NULL = all).  Per pixel, fp64 after the four loads:
//   a_c  = max(alpha, 1e-10)                    gsplat's "ED": depth / alpha.clamp(min=1e-10)
//   E    = depth / a_c
//   disp = E > 0 ? 1 / E : 0                    simple_trainer.py:958
//   used = mask && depth_gt > 0 && isfinite(depth_gt)
//   term = used ? |disp - 1 / depth_gt| : 0
//   loss = scale * sum(term) / M,  M = number of used pixels of all C cameras
// Expected depth is never materialised: the normalisation and its chain rule live in these kernels.
//
// Two deviations from the reference: a pixel whose target is not a positive finite number is skipped (the reference would divide
// by it), and M == 0 gives loss 0 and zero gradients (the reference's empty mean is NaN).
//
// Forward: one grid-stride pass, 16-byte loads of depth / alpha / depth_gt and a 4-byte load of the mask where all four pointers
// allow, a scalar tail (and everything scalar where they do not); one fp64 partial sum and one count per workgroup, then a
// one-workgroup reduction in the order of fixed_sum.h.  The grid depends on the size only: bit-identical run to run, no atomics.
// Backward: one launch, every element of d_depth and d_alpha written exactly once (zero where the pixel is unused or E <= 0), M read
// from the forward's output on the device.  With s = sign(disp - 1 / depth_gt), sign(0) = 0:
//   dL/dE = -s scale / (M E^2),   d_depth = d_out dL/dE / a_c,   d_alpha = alpha > 1e-10 ? -d_out dL/dE depth / alpha^2 : 0
// d_out multiplies a coefficient that does not depend on it: exactly linear in the incoming gradient.
// The 16-byte path is all or nothing for a call: where one pointer misses its alignment (a per-view slice [j:j+1] of a [V,H,W] map
// with H W % 4 != 0, for instance) every pixel of the call takes the scalar loop, on the same grid; the results are the same.
// HBM-bound: 13 bytes read per pixel forward, 13 read and 8 written backward.
#include "common.h"
#include "fixed_sum.h"
#include "../../include/vist3a_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 2048;      // 8 workgroups on each of the 256 CUs; the rest of the map is reached by the grid stride
constexpr double ALPHA_MIN = 1e-10;

struct DepthP {
  const float* depth; const float* alpha; const float* gt; const unsigned char* mask;
  long n, nvec;                       // pixels; 4-pixel groups moved by 16-byte accesses (0 where a pointer is not aligned)
  double scale;
};

__device__ __forceinline__ bool used_px(float gt, unsigned m) { return m != 0u && gt > 0.f && gt <= 3.402823466e+38f; }

// disparity of the expected depth; e = E and ac = the clamped alpha for the backward
__device__ __forceinline__ double disparity(float depth, float alpha, double& e, double& ac) {
  ac = fmax((double)alpha, ALPHA_MIN);
  e = (double)depth / ac;
  return e > 0.0 ? 1.0 / e : 0.0;
}

__device__ __forceinline__ void fwd_one(float depth, float alpha, float gt, unsigned m, double& sum, long long& cnt) {
  if (!used_px(gt, m)) return;
  double e, ac;
  const double disp = disparity(depth, alpha, e, ac);
  sum += fabs(disp - 1.0 / (double)gt);
  cnt += 1;
}

__global__ void __launch_bounds__(THREADS) depth_loss_fwd_kernel(const DepthP p, double* part_sum, long long* part_cnt) {
  __shared__ double red_s[THREADS];
  __shared__ long long red_c[THREADS];
  const long stride = (long)gridDim.x * THREADS;
  const long t0 = (long)blockIdx.x * THREADS + threadIdx.x;
  double sum = 0.0;
  long long cnt = 0;
  for (long v = t0; v < p.nvec; v += stride) {
    const float4 d = ((const float4*)p.depth)[v], a = ((const float4*)p.alpha)[v], g = ((const float4*)p.gt)[v];
    const unsigned m = p.mask ? ((const unsigned*)p.mask)[v] : 0x01010101u;
    fwd_one(d.x, a.x, g.x, m & 0xffu, sum, cnt);
    fwd_one(d.y, a.y, g.y, m & 0xff00u, sum, cnt);
    fwd_one(d.z, a.z, g.z, m & 0xff0000u, sum, cnt);
    fwd_one(d.w, a.w, g.w, m & 0xff000000u, sum, cnt);
  }
  for (long e = p.nvec * 4 + t0; e < p.n; e += stride)
    fwd_one(p.depth[e], p.alpha[e], p.gt[e], p.mask ? (unsigned)p.mask[e] : 1u, sum, cnt);
  const double ts = block_sum<THREADS>(sum, red_s);
  const long long tc = block_sum<THREADS>(cnt, red_c);
  if (threadIdx.x == 0) {
    part_sum[blockIdx.x] = ts;
    part_cnt[blockIdx.x] = tc;
  }
}

// out[0] = loss, out[1] = M.  One workgroup, partials in index order per lane, then the fixed tree.
__global__ void __launch_bounds__(THREADS) depth_loss_reduce_kernel(const double* part_sum, const long long* part_cnt, int parts,
                                                                     double scale, double* out) {
  __shared__ double red_s[THREADS];
  __shared__ long long red_c[THREADS];
  double s = 0.0;
  long long c = 0;
  for (int t = threadIdx.x; t < parts; t += THREADS) {
    s += part_sum[t];
    c += part_cnt[t];
  }
  const double ts = block_sum<THREADS>(s, red_s);
  const long long tc = block_sum<THREADS>(c, red_c);
  if (threadIdx.x == 0) {
    out[0] = tc > 0 ? scale * ts / (double)tc : 0.0;
    out[1] = (double)tc;
  }
}

// k = scale / M (0 when M == 0), g = d_out
__device__ __forceinline__ void bwd_one(float depth, float alpha, float gt, unsigned m, double k, double g, float& d_depth, float& d_alpha) {
  d_depth = 0.f;
  d_alpha = 0.f;
  if (!used_px(gt, m)) return;
  double e, ac;
  const double disp = disparity(depth, alpha, e, ac);
  if (!(e > 0.0)) return;
  const double diff = disp - 1.0 / (double)gt;
  const double s = diff > 0.0 ? 1.0 : (diff < 0.0 ? -1.0 : 0.0);
  const double dE = -s * k / (e * e);
  d_depth = (float)(g * (dE / ac));
  if ((double)alpha > ALPHA_MIN) d_alpha = (float)(g * (-dE * (double)depth / ((double)alpha * (double)alpha)));
}

__global__ void __launch_bounds__(THREADS) depth_loss_bwd_kernel(const DepthP p, const double* out, const double* d_out,
                                                                  float* d_depth, float* d_alpha) {
  const long stride = (long)gridDim.x * THREADS;
  const long t0 = (long)blockIdx.x * THREADS + threadIdx.x;
  const double M = out[1], g = d_out[0];
  const double k = M > 0.0 ? p.scale / M : 0.0;
  for (long v = t0; v < p.nvec; v += stride) {
    const float4 d = ((const float4*)p.depth)[v], a = ((const float4*)p.alpha)[v], t = ((const float4*)p.gt)[v];
    const unsigned m = p.mask ? ((const unsigned*)p.mask)[v] : 0x01010101u;
    float4 gd, ga;
    bwd_one(d.x, a.x, t.x, m & 0xffu, k, g, gd.x, ga.x);
    bwd_one(d.y, a.y, t.y, m & 0xff00u, k, g, gd.y, ga.y);
    bwd_one(d.z, a.z, t.z, m & 0xff0000u, k, g, gd.z, ga.z);
    bwd_one(d.w, a.w, t.w, m & 0xff000000u, k, g, gd.w, ga.w);
    ((float4*)d_depth)[v] = gd;
    ((float4*)d_alpha)[v] = ga;
  }
  for (long e = p.nvec * 4 + t0; e < p.n; e += stride) {
    float gd, ga;
    bwd_one(p.depth[e], p.alpha[e], p.gt[e], p.mask ? (unsigned)p.mask[e] : 1u, k, g, gd, ga);
    d_depth[e] = gd;
    d_alpha[e] = ga;
  }
}

bool bad_shape(int C, int H, int W) {
  return C < 1 || H < 1 || W < 1 || (long)C * H * W > 0x7fffffffL;
}

long groups(long n) { return n / 4 + n % 4; }   // one thread per 16-byte group and per tail pixel

// the grid of a call: from the size alone, also where the scalar path runs, so that workspace and summation order are fixed
DepthP params(const v3a_depth_loss_args* a, const void* o1, const void* o2) {
  DepthP p;
  p.depth = a->depth; p.alpha = a->alpha; p.gt = a->depth_gt; p.mask = a->mask;
  p.n = (long)a->C * a->H * a->W;
  const uintptr_t al = (uintptr_t)a->depth | (uintptr_t)a->alpha | (uintptr_t)a->depth_gt | (uintptr_t)o1 | (uintptr_t)o2;
  p.nvec = ((al & 15) || ((uintptr_t)a->mask & 3)) ? 0 : p.n / 4;
  p.scale = a->scale;
  return p;
}

}  // namespace

extern "C" long v3a_depth_loss_workspace_bytes(int C, int H, int W) {
  if (bad_shape(C, H, W)) return V3A_ERR_SHAPE;
  return (long)grid_blocks(groups((long)C * H * W), THREADS, MAX_BLOCKS) * (long)(sizeof(double) + sizeof(long long));
}

extern "C" int v3a_depth_loss_forward(const v3a_depth_loss_args* a, void* stream) {
  if (!a || !a->depth || !a->alpha || !a->depth_gt || !a->out) return V3A_ERR_ARG;
  if (bad_shape(a->C, a->H, a->W)) return V3A_ERR_SHAPE;
  if (!a->workspace || ((uintptr_t)a->workspace & 7) || a->workspace_bytes < v3a_depth_loss_workspace_bytes(a->C, a->H, a->W))
    return V3A_ERR_WORKSPACE;
  const DepthP p = params(a, nullptr, nullptr);
  const int blocks = grid_blocks(groups(p.n), THREADS, MAX_BLOCKS);
  double* part_sum = (double*)a->workspace;
  long long* part_cnt = (long long*)(part_sum + blocks);
  hipLaunchKernelGGL(depth_loss_fwd_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, p, part_sum, part_cnt);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(depth_loss_reduce_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, part_sum, part_cnt, blocks, p.scale, a->out);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_depth_loss_backward(const v3a_depth_loss_args* a, const double* d_out, float* d_depth, float* d_alpha, void* stream) {
  if (!a || !a->depth || !a->alpha || !a->depth_gt || !a->out || !d_out || !d_depth || !d_alpha) return V3A_ERR_ARG;
  if (bad_shape(a->C, a->H, a->W)) return V3A_ERR_SHAPE;
  const DepthP p = params(a, d_depth, d_alpha);
  hipLaunchKernelGGL(depth_loss_bwd_kernel, dim3(grid_blocks(groups(p.n), THREADS, MAX_BLOCKS)), dim3(THREADS), 0, (hipStream_t)stream, p, a->out, d_out, d_depth, d_alpha);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
