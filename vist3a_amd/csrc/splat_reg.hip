// The two regularisers of the post-optimisation loop, forward and backward (third_party_model/anysplat/src/post_opt/
// simple_trainer.py:966-977):  opacity_reg * |sigmoid(logit)|.mean()  and  scale_reg * |exp(log_scale)|.mean()  over the scene's
// opacity logits f32 [U] and log-scales f32 [U,3].  Both activations are positive, so the reference's abs() is the identity.
//
//   out[0] = sum_i sigmoid(logit_i) / U          out[1] = sum_j exp(log_scale_j) / (3 U)          (f64 [2], unweighted)
//
// Forward: one grid-stride pass over both arrays, fp64 after the loads, 16-byte loads where an array's pointer allows with a scalar
// tail (all scalar where it does not); one fp64 partial per sum and workgroup, then a one-workgroup reduction in the order of
// fixed_sum.h.  The grid depends on U only: bit-identical run to run, no atomics.
// Backward: one launch, every element of d_logits and d_log_scales written exactly once:
//   d_logit = g0 s (1 - s) / U,   d_log_scale = g1 exp(ls) / (3 U)
// g multiplies a coefficient that does not depend on it: exactly linear in the incoming gradient.
// HBM-bound: 16 bytes read per Gaussian forward, 16 read and 16 written backward.
#include "common.h"
#include "fixed_sum.h"
#include "splat_quat.h"   // sigmoid64
#include "../../include/vist3a_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 2048;      // 8 workgroups on each of the 256 CUs; the rest is reached by the grid stride

struct RegP {
  const float* logits; const float* ls;
  long n_op, n_sc;                    // U and 3 U
  long vec_op, vec_sc;                // 4-element groups of each array moved by 16-byte accesses (0 where a pointer is not aligned)
};

__global__ void __launch_bounds__(THREADS) splat_reg_fwd_kernel(const RegP p, double* part) {
  __shared__ double red[THREADS];
  const long stride = (long)gridDim.x * THREADS;
  const long t0 = (long)blockIdx.x * THREADS + threadIdx.x;
  double so = 0.0, ss = 0.0;
  for (long v = t0; v < p.vec_op; v += stride) {
    const float4 x = ((const float4*)p.logits)[v];
    so += sigmoid64(x.x); so += sigmoid64(x.y); so += sigmoid64(x.z); so += sigmoid64(x.w);
  }
  for (long e = p.vec_op * 4 + t0; e < p.n_op; e += stride) so += sigmoid64(p.logits[e]);
  for (long v = t0; v < p.vec_sc; v += stride) {
    const float4 x = ((const float4*)p.ls)[v];
    ss += exp((double)x.x); ss += exp((double)x.y); ss += exp((double)x.z); ss += exp((double)x.w);
  }
  for (long e = p.vec_sc * 4 + t0; e < p.n_sc; e += stride) ss += exp((double)p.ls[e]);
  const double to = block_sum<THREADS>(so, red);
  const double ts = block_sum<THREADS>(ss, red);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = to;
    part[2 * blockIdx.x + 1] = ts;
  }
}

// out[0] = mean opacity, out[1] = mean scale.  One workgroup, partials in index order per lane, then the fixed tree.
__global__ void __launch_bounds__(THREADS) splat_reg_reduce_kernel(const double* part, int parts, double n_op, double n_sc, double* out) {
  __shared__ double red[THREADS];
  double so = 0.0, ss = 0.0;
  for (int t = threadIdx.x; t < parts; t += THREADS) {
    so += part[2 * t];
    ss += part[2 * t + 1];
  }
  const double to = block_sum<THREADS>(so, red);
  const double ts = block_sum<THREADS>(ss, red);
  if (threadIdx.x == 0) {
    out[0] = to / n_op;
    out[1] = ts / n_sc;
  }
}

__device__ __forceinline__ float d_logit_one(float x, double g, double inv_n) {
  const double s = sigmoid64(x);
  return (float)(g * (s * (1.0 - s) * inv_n));
}

__device__ __forceinline__ float d_scale_one(float x, double g, double inv_n) { return (float)(g * (exp((double)x) * inv_n)); }

__global__ void __launch_bounds__(THREADS) splat_reg_bwd_kernel(const RegP p, const double* d_out, float* d_logits, float* d_ls) {
  const long stride = (long)gridDim.x * THREADS;
  const long t0 = (long)blockIdx.x * THREADS + threadIdx.x;
  const double g0 = d_out[0], g1 = d_out[1];
  const double io = 1.0 / (double)p.n_op, is = 1.0 / (double)p.n_sc;
  for (long v = t0; v < p.vec_op; v += stride) {
    const float4 x = ((const float4*)p.logits)[v];
    float4 d;
    d.x = d_logit_one(x.x, g0, io); d.y = d_logit_one(x.y, g0, io); d.z = d_logit_one(x.z, g0, io); d.w = d_logit_one(x.w, g0, io);
    ((float4*)d_logits)[v] = d;
  }
  for (long e = p.vec_op * 4 + t0; e < p.n_op; e += stride) d_logits[e] = d_logit_one(p.logits[e], g0, io);
  for (long v = t0; v < p.vec_sc; v += stride) {
    const float4 x = ((const float4*)p.ls)[v];
    float4 d;
    d.x = d_scale_one(x.x, g1, is); d.y = d_scale_one(x.y, g1, is); d.z = d_scale_one(x.z, g1, is); d.w = d_scale_one(x.w, g1, is);
    ((float4*)d_ls)[v] = d;
  }
  for (long e = p.vec_sc * 4 + t0; e < p.n_sc; e += stride) d_ls[e] = d_scale_one(p.ls[e], g1, is);
}

bool bad_size(long U) { return U < 1 || 3 * U > 0x7fffffffL; }

long groups(long n) { return n / 4 + n % 4; }   // one thread per 16-byte group and per tail element

// the grid of a call: from U alone (the log-scales are the longer array), also where the scalar path runs
int blocks_of(long U) { return grid_blocks(groups(3 * U), THREADS, MAX_BLOCKS); }

// o1 / o2: the backward's outputs, which share the 16-byte path of their inputs (null in the forward)
RegP params(const float* logits, const float* ls, long U, const void* o1, const void* o2) {
  RegP p;
  p.logits = logits; p.ls = ls;
  p.n_op = U; p.n_sc = 3 * U;
  p.vec_op = (((uintptr_t)logits | (uintptr_t)o1) & 15) ? 0 : p.n_op / 4;
  p.vec_sc = (((uintptr_t)ls | (uintptr_t)o2) & 15) ? 0 : p.n_sc / 4;
  return p;
}

}  // namespace

extern "C" long v3a_splat_reg_workspace_bytes(long U) {
  if (bad_size(U)) return V3A_ERR_SHAPE;
  return (long)blocks_of(U) * 2 * (long)sizeof(double);
}

extern "C" int v3a_splat_reg(const float* logits, const float* log_scales, long U, double* out, void* workspace, long workspace_bytes,
                             void* stream) {
  if (!logits || !log_scales || !out) return V3A_ERR_ARG;
  if (bad_size(U)) return V3A_ERR_SHAPE;
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < v3a_splat_reg_workspace_bytes(U)) return V3A_ERR_WORKSPACE;
  const RegP p = params(logits, log_scales, U, nullptr, nullptr);
  const int blocks = blocks_of(U);
  double* part = (double*)workspace;
  hipLaunchKernelGGL(splat_reg_fwd_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, p, part);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(splat_reg_reduce_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, part, blocks, (double)p.n_op,
                     (double)p.n_sc, out);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_splat_reg_backward(const float* logits, const float* log_scales, long U, const double* d_out, float* d_logits,
                                      float* d_log_scales, void* stream) {
  if (!logits || !log_scales || !d_out || !d_logits || !d_log_scales) return V3A_ERR_ARG;
  if (bad_size(U)) return V3A_ERR_SHAPE;
  const RegP p = params(logits, log_scales, U, d_logits, d_log_scales);
  hipLaunchKernelGGL(splat_reg_bwd_kernel, dim3(blocks_of(U)), dim3(THREADS), 0, (hipStream_t)stream, p, d_out, d_logits, d_log_scales);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
