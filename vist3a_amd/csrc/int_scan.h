// The one integer scan behind the stream compactions of the post-optimisation and export kernels: the three segment offsets of
// v3a_densify_classify (densify.hip) and the survivor list of v3a_splat_export_filter (splat_export.hip).  Both cut their rows
// into blocks of THREADS, scan every block, and let one workgroup turn the blocks' totals into their exclusive prefix.
// splat_import.hip uses the second stage alone: the sum of its workgroups' counts of non-finite rows.
// tests/test_int_scan_gpu.py pins offsets and totals through both users at one row, around one block, and around the 256 blocks
// that one round of the second stage holds.  Included by those three files only, not by common.h.
//
// Integers only: no order of the additions can change a result, so every user is bit-identical run to run.  The sums are int32;
// the entry points refuse more than 2^31 - 1 rows.
//
// Deliberately NOT built on these helpers: mcmc_prefix_kernel (mcmc.hip) adds its fp64 block weights sequentially in block order,
// and that order is part of the sampler's contract (tests/mcmc_oracle.py emulates it); the scans of voxel.hip and of the
// rasteriser are rocPRIM's device-wide scans over millions of items on the reconstruction path that the benchmark times.
#pragma once
#include "common.h"

// Exclusive prefix of x over the THREADS lanes of a workgroup (Hillis-Steele) through the caller's LDS array buf[THREADS]; `total`
// receives the workgroup's sum in every lane.  All lanes must call it.  The trailing barrier means buf may be reused (by the next
// scan, say) as soon as this returns.
template <int THREADS>
__device__ __forceinline__ int block_exclusive_scan(int x, int* buf, int& total) {
  const int tid = threadIdx.x;
  buf[tid] = x;
  __syncthreads();
  for (int off = 1; off < THREADS; off <<= 1) {
    const int t = tid >= off ? buf[tid - off] : 0;
    __syncthreads();
    buf[tid] += t;
    __syncthreads();
  }
  total = buf[THREADS - 1];
  const int r = buf[tid] - x;
  __syncthreads();
  return r;
}

// The second stage, by ONE workgroup: the block totals T[0 .. nb) become their exclusive prefix in place, THREADS blocks per round
// with a running carry.  Every lane returns the sum of all totals.  All lanes must call it.
template <int THREADS>
__device__ __forceinline__ long block_totals_to_prefix(int* T, long nb, int* buf) {
  long run = 0;
  for (long c0 = 0; c0 < nb; c0 += THREADS) {
    const long b = c0 + threadIdx.x;
    int total;
    const int ex = block_exclusive_scan<THREADS>(b < nb ? T[b] : 0, buf, total);
    if (b < nb) T[b] = (int)(run + ex);
    run += total;
  }
  return run;
}

// Blocks of the first stage over n rows = entries of the block-totals array.
template <int THREADS>
inline long scan_blocks(long n) { return blocks_for(n, THREADS); }
