// The one definition of reduction order for the fp64 loss / metric kernels (image_metrics, ssim_loss, lpips, clip, depth_loss,
// bilagrid, color_correct, splat_reg), for the block totals of the MCMC sampler (mcmc) and for the camera-gradient finish of the
// rasteriser's backward (raster_bwd), for the moments of the principal-axes step (splat_transform), and - on integers - for the
// count of non-finite rows of a workgroup of the scene import (splat_import): what their "no atomics, fixed order, bit-identical run to run" rests on.
// tests/test_fixed_sum_gpu.py pins the order bit for bit (and tests/test_mcmc_gpu.py holds the sampler to a host emulation of
// it).  Included by those twelve files only, not by common.h.
//
// Deliberately NOT built on these helpers, because moving them onto the tree would change bits: the batched trees of
// cc_accumulate_kernel (11 wide) and bilagrid_slice_bwd_grid_kernel (12 wide), the single-thread sequential finishes
// cc_finish_kernel and mse_finish_kernel, the column sums of cc_solve_kernel, and group_sum (a shuffle butterfly) in lpips.hip.
// The second stage of the two-launch reductions - each lane adds the partials tid, tid + THREADS, ... in index order, then
// block_sum - stays written out in the five *_reduce_kernel: a shared per-array loop was tried and split the loops that add two
// arrays in one pass, which serialised their loads (+0.5 us on a 21 us call, measured).
#pragma once

// Sum of v over the THREADS lanes of a workgroup through the caller's LDS array red[THREADS].  Order: the halving tree
// red[t] += red[t + s] for s = THREADS / 2, ..., 1, i.e. lane t first meets lane t + THREADS / 2.  Every lane returns the total,
// and the trailing barrier means red may be reused (by the next block_sum, say) as soon as this returns.  All lanes must call it.
template <int THREADS, typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
#pragma unroll
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const T r = red[0];
  __syncthreads();
  return r;
}

// Workgroups of a grid-stride first stage over n items: ceil(n / threads) clamped to [1, max_blocks].  From the size alone, so that
// the workspace and the summation order of a call are fixed.
inline int grid_blocks(long n, int threads, int max_blocks) {
  const long need = (n + threads - 1) / threads;
  return (int)(need < 1 ? 1 : (need > max_blocks ? max_blocks : need));
}
