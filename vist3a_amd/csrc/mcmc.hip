// The MCMC strategy of the post-optimisation loop ("3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat's MCMCStrategy, which
// third_party_model/anysplat/src/post_opt/simple_trainer.py:1142-1150 calls in its `mcmc` configuration).  DESIGN.md section 7f
// restates the algorithm; that text, not gsplat's code, is the contract.  Three entry points:
//
//   v3a_mcmc_sample     a reproducible weighted sampler: slot s draws a Gaussian with probability proportional to its opacity.
//                       Counter-based random numbers (Philox4x32-10, no state), every sum in fp64 on exactly converted f32 values
//                       in a fixed order, so that a host emulation gives the same integers (tests/mcmc_oracle.py).
//   v3a_mcmc_relocate   dead rows take a sampled live row's place (relocation) or new rows are appended (growth); the source's
//                       opacity and scales are split over its copies (compute_relocation).  Two launches: per-source values into
//                       a scratch array first, then every row written by exactly one thread - no read-after-write race.
//   v3a_mcmc_noise      the per-step hot path: means += cov . (normal draw * gate(opacity) * scaler), one thread per Gaussian,
//                       fp64 after the loads, one rounding at the store.  44 bytes read and 12 written per Gaussian.
//
// Integer atomic adds on `counts` only (they commute); no floating-point atomics.  Nothing is read back to the host.
#include "common.h"
#include "fixed_sum.h"
#include "splat_quat.h"
#include "splat_scene.h"
#include "../../include/vist3a_hip.h"

// Below this line only: quat_R<double> of splat_quat.h is defined above it and may be contracted to FMAs, as it is in post_opt.hip.
// Nothing bit-exact depends on that (the sampler does not use it; the noise is held to 1.2e-7).
#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int PER_LANE = 4;
constexpr long BLOCK_ELEMS = (long)THREADS * PER_LANE;   // 1024 consecutive Gaussians per sampler block
constexpr int MAX_RATIO = 51;                            // gsplat's n_max: binomials up to C(50, k)

#include "philox.h"   // Rand4, philox4x32_10, uniform53, Key, draw, normal_pair, make_key

// ---------------------------------------------------------------------------------------------------------------- sampler

// the weight a Gaussian puts into the pool: relocation draws among the live ones only
__device__ __forceinline__ double pool_weight(float w, float min_w, int alive_only) {
  return (alive_only && !(w > min_w)) ? 0.0 : (double)w;
}

// T[b] = the pool weight of block b: each lane adds its 4 consecutive elements in index order, then the tree of fixed_sum.h.
// Also zeroes counts.
__global__ void __launch_bounds__(THREADS) mcmc_totals_kernel(const float* __restrict__ w, long U, float min_w, int alive_only,
                                                              double* __restrict__ T, int* __restrict__ counts) {
  __shared__ double red[THREADS];
  const long base = (long)blockIdx.x * BLOCK_ELEMS + (long)threadIdx.x * PER_LANE;
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < PER_LANE; ++e) {
    const long i = base + e;
    if (i < U) {
      s += pool_weight(w[i], min_w, alive_only);
      counts[i] = 0;
    }
  }
  const double t = block_sum<THREADS>(s, red);
  if (threadIdx.x == 0) T[blockIdx.x] = t;
}

// P[b] = T[0] + ... + T[b - 1], added sequentially in block order by one lane (the others stage T through LDS); *total = the sum of all.
__global__ void __launch_bounds__(THREADS) mcmc_prefix_kernel(const double* __restrict__ T, long nb, double* __restrict__ P,
                                                              double* __restrict__ total) {
  __shared__ double buf[THREADS];
  double run = 0.0;
  for (long c = 0; c < nb; c += THREADS) {
    const long b = c + threadIdx.x;
    buf[threadIdx.x] = b < nb ? T[b] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = (int)(nb - c < THREADS ? nb - c : THREADS);
      for (int k = 0; k < n; ++k) {
        P[c + k] = run;
        run += buf[k];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *total = run;
}

// One thread per slot.  An inactive slot (relocation: a live Gaussian) and every slot of an empty pool get src = -1.
__global__ void __launch_bounds__(THREADS) mcmc_pick_kernel(const float* __restrict__ w, long U, float min_w, int alive_only, long n_slots,
                                                            Key key, const double* __restrict__ T, const double* __restrict__ P,
                                                            const double* __restrict__ total_p, long nb, int* __restrict__ src,
                                                            int* __restrict__ counts) {
  const long s = (long)blockIdx.x * THREADS + threadIdx.x;
  if (s >= n_slots) return;
  const double total = *total_p;
  if ((alive_only && w[s] > min_w) || !(total > 0.0)) {
    src[s] = -1;
    return;
  }
  const Rand4 r = draw(key, (uint32_t)s, key.stream);
  const double t = uniform53(r.x[0], r.x[1]) * total;
  long lo = 0, hi = nb - 1;              // the last block with P[b] <= t (P[0] = 0 <= t, P does not decrease) ...
  while (lo < hi) {
    const long mid = (lo + hi + 1) / 2;
    if (P[mid] <= t) lo = mid; else hi = mid - 1;
  }
  while (lo > 0 && !(T[lo] > 0.0)) --lo;   // ... that holds any weight
  const long i0 = lo * BLOCK_ELEMS, i1 = i0 + BLOCK_ELEMS < U ? i0 + BLOCK_ELEMS : U;
  double c = P[lo];
  long pick = -1;
  for (long i = i0; i < i1; ++i) {
    const double wi = pool_weight(w[i], min_w, alive_only);
    if (wi > 0.0) {
      c += wi;
      pick = i;                            // the block's last weighted element, should rounding leave c <= t to the end
      if (c > t) break;
    }
  }
  src[s] = (int)pick;
  if (pick >= 0) atomicAdd(&counts[pick], 1);
}

long sample_blocks(long U) { return (U + BLOCK_ELEMS - 1) / BLOCK_ELEMS; }

// ------------------------------------------------------------------------------------------------- relocation and growth

struct MoveP {
  const int* src; const int* counts;
  SplatSet<float> p, m, v; int n_sh;       // n_sh: floats per harmonics row, 3 K
  long U, n_slots, dst_offset;
  double min_opacity;
  float* scratch;                          // [U, 4]: the new (logit, log-scales) of every source
};

// compute_relocation for source j drawn counts[j] times: its opacity and scales split over counts[j] + 1 copies.
__global__ void __launch_bounds__(THREADS) mcmc_new_values_kernel(const MoveP a) {
  const long j = (long)blockIdx.x * THREADS + threadIdx.x;
  if (j >= a.U) return;
  const int cnt = a.counts[j];
  if (cnt < 1) return;
  const int r = cnt + 1 < MAX_RATIO ? cnt + 1 : MAX_RATIO;
  const double op = sigmoid64(a.p[SPLAT_LOGITS][j]);
  const double o1 = 1.0 - pow(1.0 - op, 1.0 / (double)r);
  double den = 0.0;
  for (int i = 1; i <= r; ++i) {
    double binom = 1.0, pw = o1, sign = 1.0;     // C(i - 1, k), o1^(k + 1), (-1)^k
    for (int k = 0; k < i; ++k) {
      den += binom * (sign / sqrt((double)(k + 1))) * pw;
      binom = binom * (double)(i - 1 - k) / (double)(k + 1);   // exact: integers below 2^53, the quotient an integer
      pw *= o1;
      sign = -sign;
    }
  }
  const double coef = op / den;
  const double hi = 1.0 - 1.0 / 8388608.0;
  const double o2 = o1 < a.min_opacity ? a.min_opacity : (o1 > hi ? hi : o1);
  a.scratch[j * 4] = (float)log(o2 / (1.0 - o2));
#pragma unroll
  for (int e = 0; e < 3; ++e) a.scratch[j * 4 + 1 + e] = (float)log(coef * exp((double)a.p[SPLAT_LS][j * 3 + e]));
}

// both moments of row r in all five tensors
__device__ __forceinline__ void zero_moments(const MoveP& a, long r) {
  for (int f = 0; f < SPLAT_FIELDS; ++f)
    for (int e = 0, w = splat_width(f, a.n_sh); e < w; ++e) a.m[f][r * w + e] = a.v[f][r * w + e] = 0.f;
}

// Threads [0, U): row j as a source takes its new values (and, relocating, loses its moments).  Threads [U, U + n_slots): slot s
// fills row dst_offset + s from its source (and, growing, starts with zero moments).  Sources and destinations are disjoint rows.
__global__ void __launch_bounds__(THREADS) mcmc_move_kernel(const MoveP a) {
  const long t = (long)blockIdx.x * THREADS + threadIdx.x;
  const bool growth = a.dst_offset != 0;
  if (t < a.U) {
    const long j = t;
    if (a.counts[j] < 1) return;
    a.p[SPLAT_LOGITS][j] = a.scratch[j * 4];
#pragma unroll
    for (int e = 0; e < 3; ++e) a.p[SPLAT_LS][j * 3 + e] = a.scratch[j * 4 + 1 + e];
    if (!growth) zero_moments(a, j);
    return;
  }
  const long s = t - a.U;
  if (s >= a.n_slots) return;
  const long j = a.src[s];
  if (j < 0 || j >= a.U || a.counts[j] < 1) return;
  const long d = a.dst_offset + s;
  a.p[SPLAT_LOGITS][d] = a.scratch[j * 4];
#pragma unroll
  for (int e = 0; e < 3; ++e) a.p[SPLAT_LS][d * 3 + e] = a.scratch[j * 4 + 1 + e];
#pragma unroll
  for (int e = 0; e < 3; ++e) a.p[SPLAT_MEANS][d * 3 + e] = a.p[SPLAT_MEANS][j * 3 + e];
#pragma unroll
  for (int e = 0; e < 4; ++e) a.p[SPLAT_QUATS][d * 4 + e] = a.p[SPLAT_QUATS][j * 4 + e];
  for (int e = 0; e < a.n_sh; ++e) a.p[SPLAT_SH][d * a.n_sh + e] = a.p[SPLAT_SH][j * a.n_sh + e];
  if (growth) zero_moments(a, d);
}

// ------------------------------------------------------------------------------------------------------------------ noise

// One thread per Gaussian.  quat_vec: the quaternions' pointer is 16-byte aligned and a row is one 16-byte load.
__global__ void __launch_bounds__(THREADS) mcmc_noise_kernel(float* __restrict__ means, const float* __restrict__ log_scales,
                                                             const float* __restrict__ quats, const float* __restrict__ logits, long U,
                                                             double scaler, Key key, int quat_vec) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= U) return;
  double q[4], R[9], s2[3], mu[3];
  if (quat_vec) {
    const float4 v = ((const float4*)quats)[i];
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = quats[i * 4 + e];
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    s2[e] = exp(2.0 * (double)log_scales[i * 3 + e]);
    mu[e] = means[i * 3 + e];
  }
  const double op = sigmoid64(logits[i]);
  const double gate = 1.0 / (1.0 + exp(-100.0 * ((1.0 - op) - 0.995)));
  quat_R<double>(q, R);
  double n[3], unused;
  normal_pair(draw(key, (uint32_t)i, 2u), n[0], n[1]);
  normal_pair(draw(key, (uint32_t)i, 3u), n[2], unused);
  const double g = gate * scaler;
#pragma unroll
  for (int e = 0; e < 3; ++e) n[e] *= g;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double d = 0.0;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      double cov = 0.0;
#pragma unroll
      for (int m = 0; m < 3; ++m) cov += (R[a * 3 + m] * s2[m]) * R[b * 3 + m];
      d += cov * n[b];
    }
    means[i * 3 + a] = (float)(mu[a] + d);
  }
}

}  // namespace

extern "C" int v3a_mcmc_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  if (!counter || !key || !out) return V3A_ERR_ARG;
  const Rand4 r = philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
  for (int e = 0; e < 4; ++e) out[e] = r.x[e];
  return V3A_OK;
}

extern "C" double v3a_mcmc_uniform(uint32_t x0, uint32_t x1) { return uniform53(x0, x1); }

extern "C" long v3a_mcmc_sample_workspace_bytes(long U) {
  if (U < 1 || bad_count(U)) return V3A_ERR_SHAPE;
  return (2 * sample_blocks(U) + 1) * (long)sizeof(double);
}

extern "C" int v3a_mcmc_sample(const float* weights, long U, float min_weight, int alive_only, long n_slots, unsigned long long seed,
                               unsigned int rng_stream, unsigned int step, int* src, int* counts, void* workspace, long workspace_bytes,
                               void* stream) {
  if (!weights || !src || !counts) return V3A_ERR_ARG;
  if (U < 1 || bad_count(U) || n_slots < 1 || bad_count(n_slots) || (alive_only && n_slots != U)) return V3A_ERR_SHAPE;
  if (bad_workspace(workspace, workspace_bytes, v3a_mcmc_sample_workspace_bytes(U))) return V3A_ERR_WORKSPACE;
  const long nb = sample_blocks(U);
  double* T = (double*)workspace;
  double* P = T + nb;
  double* total = P + nb;
  const Key key = make_key(seed, rng_stream, step);
  hipLaunchKernelGGL(mcmc_totals_kernel, dim3((unsigned)nb), dim3(THREADS), 0, (hipStream_t)stream, weights, U, min_weight, alive_only, T, counts);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(mcmc_prefix_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, T, nb, P, total);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(mcmc_pick_kernel, dim3(blocks_for(n_slots, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, weights, U, min_weight, alive_only,
                     n_slots, key, T, P, total, nb, src, counts);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" long v3a_mcmc_relocate_workspace_bytes(long U) {
  if (U < 1 || bad_count(U)) return V3A_ERR_SHAPE;
  return U * 4 * (long)sizeof(float);
}

extern "C" int v3a_mcmc_relocate(const v3a_mcmc_relocate_args* a, void* stream) {
  if (!a || !a->src || !a->counts) return V3A_ERR_ARG;
  const SplatSet<float> g[SPLAT_GROUPS] = {SPLAT_SET(a, ), SPLAT_SET(a, m_), SPLAT_SET(a, v_)};
  if (splat_sets_have_null(g)) return V3A_ERR_ARG;
  if (a->U < 1 || bad_count(a->U) || a->n_slots < 1 || bad_count(a->n_slots) || a->K < 1 || a->K > 1024) return V3A_ERR_SHAPE;
  if (a->dst_offset == 0 ? a->n_slots != a->U : a->dst_offset != a->U) return V3A_ERR_SHAPE;   // relocation : growth
  if (a->dst_offset + a->n_slots > 0x7fffffffL) return V3A_ERR_SHAPE;
  if (!(a->min_opacity > 0.0) || !(a->min_opacity < 1.0)) return V3A_ERR_SHAPE;
  if (bad_workspace(a->workspace, a->workspace_bytes, v3a_mcmc_relocate_workspace_bytes(a->U))) return V3A_ERR_WORKSPACE;
  MoveP k;
  k.src = a->src; k.counts = a->counts;
  k.p = g[SPLAT_PARAMS]; k.m = g[SPLAT_M]; k.v = g[SPLAT_V]; k.n_sh = 3 * a->K;
  k.U = a->U; k.n_slots = a->n_slots; k.dst_offset = a->dst_offset;
  k.min_opacity = a->min_opacity;
  k.scratch = (float*)a->workspace;
  hipLaunchKernelGGL(mcmc_new_values_kernel, dim3(blocks_for(k.U, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, k);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(mcmc_move_kernel, dim3(blocks_for(k.U + k.n_slots, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, k);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_mcmc_noise(float* means, const float* log_scales, const float* quats, const float* logits, long U, double scaler,
                              unsigned long long seed, unsigned int step, void* stream) {
  if (!means || !log_scales || !quats || !logits) return V3A_ERR_ARG;
  if (U < 1 || bad_count(U)) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(mcmc_noise_kernel, dim3(blocks_for(U, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, means, log_scales, quats, logits, U,
                     scaler, make_key(seed, 0u, step), ((uintptr_t)quats & 15) ? 0 : 1);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
