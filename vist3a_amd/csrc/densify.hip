// Adaptive density control of the post-optimisation loop (the classic 3DGS densification; gsplat's DefaultStrategy, around which
// third_party_model/anysplat/src/post_opt/simple_trainer.py builds its `default` configuration, :1486-1491).  DESIGN.md section 7f
// restates the algorithm; that text, not gsplat's code, is the contract.  Four entry points:
//
//   v3a_densify_accumulate     every step: the screen-space gradient norm of every visible (camera, Gaussian) entry joins the
//                              Gaussian's running sum.  One thread per Gaussian, cameras in index order, fp64 norm and sum, one
//                              rounding per call.  28 bytes per Gaussian at one camera.
//   v3a_densify_classify       every refine: a fate byte per parent (keep / clone / split, pruned or not; fp64 decisions) and the
//                              rows it leaves in each output segment, then the exclusive prefix sums of those three count arrays
//                              (blocks of 256, block totals scanned in order by one workgroup per array) and their totals.
//   v3a_densify_apply          every refine: the fifteen new tensors from the old ones.  Every output row belongs to exactly one
//                              parent, so every element is written exactly once by plain stores: no memset, no atomics.  Two
//                              launches: the 11-float rows (one thread per parent; split children draw their offsets here) and
//                              the harmonics rows (16 lanes per parent).
//   v3a_densify_reset_opacity  elementwise cap of the logits, zeroing their moments.
//
// Integers only in the scans, fixed order everywhere else: results are bit-identical run to run.
#include "common.h"
#include "int_scan.h"
#include "splat_quat.h"
#include "splat_scene.h"
#include "../../include/vist3a_hip.h"

// Below this line only (as in mcmc.hip): quat_R<double> is defined above it and may be contracted; the child means are held to 2^-23.
#pragma clang fp contract(off)

namespace {

#include "philox.h"

constexpr int THREADS = 256;
constexpr int SH_LANES = 16;                       // lanes that move one parent's harmonics rows
constexpr int KEEP = 0, CLONE = 1, SPLIT = 2, PRUNED = 4;
constexpr double LOG_1_6 = 0.47000362924573555;    // log(1.6)

// -------------------------------------------------------------------------------------------------------------- accumulate

__global__ void __launch_bounds__(THREADS) densify_accumulate_kernel(const float* __restrict__ d_means2d, const int* __restrict__ radii, long U,
                                                                     int C, double sx, double sy, float* __restrict__ grad2d,
                                                                     int* __restrict__ count) {
  const long g = (long)blockIdx.x * THREADS + threadIdx.x;
  if (g >= U) return;
  double s = 0.0;
  int n = 0;
  for (int c = 0; c < C; ++c) {
    const long e = (long)c * U + g;
    if (radii[e] > 0) {
      const double gx = (double)d_means2d[2 * e] * sx, gy = (double)d_means2d[2 * e + 1] * sy;
      s += sqrt(gx * gx + gy * gy);
      ++n;
    }
  }
  if (n > 0) {
    grad2d[g] = (float)((double)grad2d[g] + s);
    count[g] += n;
  }
}

// ---------------------------------------------------------------------------------------------------------------- classify

struct ClassP {
  const float* grad2d; const int* count; const float* ls; const float* logits;
  long U, nb;
  double grow_grad2d, grow_scale3d, prune_opa, prune_scale3d;
  int grow, prune_big, revised;
  unsigned char* fates; int* counts; int* offsets; long* totals;
  int* block_tot;   // [3, nb]: the blocks' totals, then (in place) their exclusive prefix
};

// the fate byte and the three counts of every parent; a block's exclusive prefix goes to offsets, its totals to block_tot
__global__ void __launch_bounds__(THREADS) densify_classify_kernel(const ClassP a) {
  __shared__ int buf[THREADS];
  const long g = (long)blockIdx.x * THREADS + threadIdx.x;
  int c[3] = {0, 0, 0};
  if (g < a.U) {
    double smax = exp((double)a.ls[3 * g]);
#pragma unroll
    for (int k = 1; k < 3; ++k) {
      const double s = exp((double)a.ls[3 * g + k]);
      smax = s > smax ? s : smax;
    }
    const int cnt = a.count[g];
    const double avg = (double)a.grad2d[g] / (double)(cnt > 1 ? cnt : 1);
    int fate = KEEP;
    if (a.grow && avg > a.grow_grad2d) fate = smax <= a.grow_scale3d ? CLONE : SPLIT;
    double o = sigmoid64(a.logits[g]), sc = smax;
    if (fate == SPLIT) {
      if (a.revised) o = 1.0 - sqrt(1.0 - o);
      sc = smax / 1.6;
    }
    const bool pruned = o < a.prune_opa || (a.prune_big && sc > a.prune_scale3d);
    a.fates[g] = (unsigned char)(fate | (pruned ? PRUNED : 0));
    c[0] = fate != SPLIT && !pruned;
    c[1] = fate == CLONE && !pruned;
    c[2] = fate == SPLIT && !pruned;
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    int total;
    const int ex = block_exclusive_scan<THREADS>(c[s], buf, total);
    if (g < a.U) {
      a.counts[s * a.U + g] = c[s];
      a.offsets[s * a.U + g] = ex;
    }
    if (threadIdx.x == 0) a.block_tot[s * a.nb + blockIdx.x] = total;
  }
}

// workgroup s: block_tot[s] becomes its exclusive prefix; totals[s] = the sum
__global__ void __launch_bounds__(THREADS) densify_block_prefix_kernel(const ClassP a) {
  __shared__ int buf[THREADS];
  const long run = block_totals_to_prefix<THREADS>(a.block_tot + (long)blockIdx.x * a.nb, a.nb, buf);
  if (threadIdx.x == 0) a.totals[blockIdx.x] = run;
}

__global__ void __launch_bounds__(THREADS) densify_offsets_kernel(const ClassP a) {
  const long g = (long)blockIdx.x * THREADS + threadIdx.x;
  if (g >= a.U) return;
#pragma unroll
  for (int s = 0; s < 3; ++s) a.offsets[s * a.U + g] += a.block_tot[s * a.nb + blockIdx.x];
}

// ------------------------------------------------------------------------------------------------------------------- apply

struct ApplyP {
  SplatSet<const float> o[SPLAT_GROUPS]; SplatSet<float> n[SPLAT_GROUPS];   // the old and the new [group][field]
  const unsigned char* fates; const int* offsets; const long* totals;
  long U, U_out;
  int K;
  Key key;
  int revised;
};

// the output rows of parent g: r[0] (an original, or the first child) and r[1] (a clone, or the second child); -> how many
__device__ __forceinline__ int dest_rows(const ApplyP& a, long g, int& fate, long* r) {
  const int fb = a.fates[g];
  fate = fb & 3;
  if (fb & PRUNED) return 0;
  const long tA = a.totals[0], tB = a.totals[1], tC = a.totals[2];
  int n;
  if (fate == SPLIT) {
    r[0] = tA + tB + a.offsets[2 * a.U + g];
    r[1] = r[0] + tC;
    n = 2;
  } else {
    r[0] = a.offsets[g];
    r[1] = tA + a.offsets[a.U + g];
    n = fate == CLONE ? 2 : 1;
  }
  for (int d = 0; d < n; ++d)
    if (r[d] < 0 || r[d] >= a.U_out) return 0;   // fates / offsets that are not classify's for these tensors: write nothing
  return n;
}

// One thread per parent: means, log-scales, quaternions and logits of its rows, and their moments.
__global__ void __launch_bounds__(THREADS) densify_rows_kernel(const ApplyP a) {
  const long g = (long)blockIdx.x * THREADS + threadIdx.x;
  if (g >= a.U) return;
  int fate;
  long r[2];
  const int n = dest_rows(a, g, fate, r);
  if (n == 0) return;
  float p[SPLAT_SH][4];
#pragma unroll
  for (int f = 0; f < SPLAT_SH; ++f)
#pragma unroll
    for (int e = 0, w = splat_width(f, 0); e < w; ++e) p[f][e] = a.o[SPLAT_PARAMS][f][g * w + e];
  if (fate != SPLIT) {
#pragma unroll
    for (int f = 0; f < SPLAT_SH; ++f)
#pragma unroll
      for (int e = 0, w = splat_width(f, 0); e < w; ++e) {
        a.n[SPLAT_PARAMS][f][r[0] * w + e] = p[f][e];
        a.n[SPLAT_M][f][r[0] * w + e] = a.o[SPLAT_M][f][g * w + e];
        a.n[SPLAT_V][f][r[0] * w + e] = a.o[SPLAT_V][f][g * w + e];
        if (n == 2) {
          a.n[SPLAT_PARAMS][f][r[1] * w + e] = p[f][e];
          a.n[SPLAT_M][f][r[1] * w + e] = 0.f;
          a.n[SPLAT_V][f][r[1] * w + e] = 0.f;
        }
      }
    return;
  }
  double q[4], R[9], sc[3];
#pragma unroll
  for (int e = 0; e < 4; ++e) q[e] = p[SPLAT_QUATS][e];
  quat_R<double>(q, R);
  float child_ls[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    sc[e] = exp((double)p[SPLAT_LS][e]);
    child_ls[e] = (float)((double)p[SPLAT_LS][e] - LOG_1_6);
  }
  float child_logit = p[SPLAT_LOGITS][0];
  if (a.revised) {
    const double o2 = 1.0 - sqrt(1.0 - sigmoid64(p[SPLAT_LOGITS][0]));
    child_logit = (float)log(o2 / (1.0 - o2));
  }
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    double z[3], unused;
    normal_pair(draw(a.key, (uint32_t)g, 4u + 2u * d), z[0], z[1]);
    normal_pair(draw(a.key, (uint32_t)g, 5u + 2u * d), z[2], unused);
#pragma unroll
    for (int e = 0; e < 3; ++e) z[e] *= sc[e];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double off = (R[3 * i] * z[0] + R[3 * i + 1] * z[1]) + R[3 * i + 2] * z[2];
      a.n[SPLAT_PARAMS][SPLAT_MEANS][r[d] * 3 + i] = (float)((double)p[SPLAT_MEANS][i] + off);
      a.n[SPLAT_PARAMS][SPLAT_LS][r[d] * 3 + i] = child_ls[i];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) a.n[SPLAT_PARAMS][SPLAT_QUATS][r[d] * 4 + e] = p[SPLAT_QUATS][e];
    a.n[SPLAT_PARAMS][SPLAT_LOGITS][r[d]] = child_logit;
#pragma unroll
    for (int f = 0; f < SPLAT_SH; ++f)
#pragma unroll
      for (int e = 0, w = splat_width(f, 0); e < w; ++e) {
        a.n[SPLAT_M][f][r[d] * w + e] = 0.f;
        a.n[SPLAT_V][f][r[d] * w + e] = 0.f;
      }
  }
}

// W floats from src to dst by SH_LANES lanes (src == nullptr: zeros).  16-byte accesses when the two pointers share their phase
// within 16 bytes (for zeros: always), after a scalar head up to dst's alignment and before a scalar tail; all scalar otherwise.
__device__ __forceinline__ void move_row(const float* __restrict__ src, float* __restrict__ dst, int W, int lane) {
  const bool vec = !src || ((((uintptr_t)src ^ (uintptr_t)dst) & 15) == 0);
  int head = vec ? (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2) : W;
  head = head < W ? head : W;
  for (int e = lane; e < head; e += SH_LANES) dst[e] = src ? src[e] : 0.f;
  if (!vec) return;
  const int nv = (W - head) >> 2;
  f32x4* d4 = (f32x4*)(dst + head);
  const f32x4* s4 = src ? (const f32x4*)(src + head) : nullptr;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int i = lane; i < nv; i += SH_LANES) d4[i] = src ? s4[i] : zero;
  for (int e = head + 4 * nv + lane; e < W; e += SH_LANES) dst[e] = src ? src[e] : 0.f;
}

// SH_LANES lanes per parent: the harmonics rows of its output rows, and their moments (copied for an original, zero otherwise)
__global__ void __launch_bounds__(THREADS) densify_sh_kernel(const ApplyP a) {
  const long g = ((long)blockIdx.x * THREADS + threadIdx.x) / SH_LANES;
  const int lane = threadIdx.x % SH_LANES;
  if (g >= a.U) return;
  int fate;
  long r[2];
  const int n = dest_rows(a, g, fate, r);
  const long W = 3L * a.K;
  for (int d = 0; d < n; ++d) {
    const bool original = d == 0 && fate != SPLIT;
    move_row(a.o[SPLAT_PARAMS][SPLAT_SH] + g * W, a.n[SPLAT_PARAMS][SPLAT_SH] + r[d] * W, (int)W, lane);
    move_row(original ? a.o[SPLAT_M][SPLAT_SH] + g * W : nullptr, a.n[SPLAT_M][SPLAT_SH] + r[d] * W, (int)W, lane);
    move_row(original ? a.o[SPLAT_V][SPLAT_SH] + g * W : nullptr, a.n[SPLAT_V][SPLAT_SH] + r[d] * W, (int)W, lane);
  }
}

// ------------------------------------------------------------------------------------------------------------------- reset

__global__ void __launch_bounds__(THREADS) densify_reset_kernel(float* __restrict__ logits, float* __restrict__ m, float* __restrict__ v,
                                                                long U, double max_opacity) {
  const long g = (long)blockIdx.x * THREADS + threadIdx.x;
  if (g >= U) return;
  const double cap = log(max_opacity / (1.0 - max_opacity));
  if ((double)logits[g] > cap) logits[g] = (float)cap;
  m[g] = 0.f;
  v[g] = 0.f;
}

bool overlap(const float* x, long nx, const float* y, long ny) {
  const uintptr_t a0 = (uintptr_t)x, a1 = a0 + 4 * (uintptr_t)nx, b0 = (uintptr_t)y, b1 = b0 + 4 * (uintptr_t)ny;
  return nx > 0 && ny > 0 && a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" int v3a_densify_accumulate(const float* d_means2d, const int* radii, long U, int C, int width, int height, float* grad2d,
                                      int* count, void* stream) {
  if (!d_means2d || !radii || !grad2d || !count) return V3A_ERR_ARG;
  if (bad_count(U) || C < 1 || width < 1 || height < 1) return V3A_ERR_SHAPE;
  if (U == 0) return V3A_OK;
  hipLaunchKernelGGL(densify_accumulate_kernel, dim3(blocks_for(U, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, d_means2d, radii, U, C,
                     0.5 * (double)width * (double)C, 0.5 * (double)height * (double)C, grad2d, count);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" long v3a_densify_classify_workspace_bytes(long U) {
  if (bad_count(U)) return V3A_ERR_SHAPE;
  return ((3 * scan_blocks<THREADS>(U) * (long)sizeof(int) + 7) / 8) * 8;
}

extern "C" int v3a_densify_classify(const v3a_densify_classify_args* a, void* stream) {
  if (!a) return V3A_ERR_ARG;
  if (bad_count(a->U)) return V3A_ERR_SHAPE;
  if (a->U == 0) return V3A_OK;
  if (!a->grad2d || !a->count || !a->log_scales || !a->logits || !a->fates || !a->counts || !a->offsets || !a->totals) return V3A_ERR_ARG;
  if (bad_workspace(a->workspace, a->workspace_bytes, v3a_densify_classify_workspace_bytes(a->U))) return V3A_ERR_WORKSPACE;
  ClassP k;
  k.grad2d = a->grad2d; k.count = a->count; k.ls = a->log_scales; k.logits = a->logits;
  k.U = a->U; k.nb = scan_blocks<THREADS>(a->U);
  k.grow_grad2d = a->grow_grad2d; k.grow_scale3d = a->grow_scale3d; k.prune_opa = a->prune_opa; k.prune_scale3d = a->prune_scale3d;
  k.grow = a->grow; k.prune_big = a->prune_big; k.revised = a->revised_opacity;
  k.fates = a->fates; k.counts = a->counts; k.offsets = a->offsets; k.totals = a->totals;
  k.block_tot = (int*)a->workspace;
  hipLaunchKernelGGL(densify_classify_kernel, dim3((unsigned)k.nb), dim3(THREADS), 0, (hipStream_t)stream, k);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(densify_block_prefix_kernel, dim3(3), dim3(THREADS), 0, (hipStream_t)stream, k);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(densify_offsets_kernel, dim3((unsigned)k.nb), dim3(THREADS), 0, (hipStream_t)stream, k);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_densify_apply(const v3a_densify_apply_args* a, void* stream) {
  if (!a) return V3A_ERR_ARG;
  if (bad_count(a->U) || bad_count(a->U_out) || a->K < 1 || a->K > 1024 || a->U_out > 2 * a->U) return V3A_ERR_SHAPE;
  if (a->U == 0 || a->U_out == 0) return V3A_OK;
  ApplyP k = {{SPLAT_SET(a, ), SPLAT_SET(a, m_), SPLAT_SET(a, v_)}, {SPLAT_SET(a, new_), SPLAT_SET(a, new_m_), SPLAT_SET(a, new_v_)}};
  if (!a->fates || !a->offsets || !a->totals || splat_sets_have_null(k.o) || splat_sets_have_null(k.n)) return V3A_ERR_ARG;
  for (int i = 0; i < SPLAT_GROUPS * SPLAT_FIELDS; ++i)
    for (int j = 0; j < SPLAT_GROUPS * SPLAT_FIELDS; ++j) {
      const int fi = i % SPLAT_FIELDS, fj = j % SPLAT_FIELDS;
      const long wi = splat_width(fi, 3 * a->K), wj = splat_width(fj, 3 * a->K);
      const float *ni = k.n[i / SPLAT_FIELDS][fi], *nj = k.n[j / SPLAT_FIELDS][fj], *oj = k.o[j / SPLAT_FIELDS][fj];
      if (overlap(ni, a->U_out * wi, oj, a->U * wj)) return V3A_ERR_SHAPE;
      if (i != j && overlap(ni, a->U_out * wi, nj, a->U_out * wj)) return V3A_ERR_SHAPE;
    }
  k.fates = a->fates; k.offsets = a->offsets; k.totals = a->totals;
  k.U = a->U; k.U_out = a->U_out; k.K = a->K;
  k.key = make_key(a->seed, 0u, a->step);   // Key.stream is the sampler's; the children name their streams (4-7) at each draw
  k.revised = a->revised_opacity;
  hipLaunchKernelGGL(densify_rows_kernel, dim3(blocks_for(k.U, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, k);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(densify_sh_kernel, dim3(blocks_for(k.U * SH_LANES, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, k);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_densify_reset_opacity(float* logits, float* m_logits, float* v_logits, long U, double max_opacity, void* stream) {
  if (!logits || !m_logits || !v_logits) return V3A_ERR_ARG;
  if (bad_count(U) || !(max_opacity > 0.0) || !(max_opacity < 1.0)) return V3A_ERR_SHAPE;
  if (U == 0) return V3A_OK;
  hipLaunchKernelGGL(densify_reset_kernel, dim3(blocks_for(U, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, logits, m_logits, v_logits, U, max_opacity);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
