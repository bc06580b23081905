// Scene export packed on the device: the compressed PLY (SuperSplat), the 32-byte .splat (antimatter15) and the plain float PLY of
// third_party_model/anysplat/src/post_opt/exporter.py (export_splats, :475-553).  DESIGN.md section 7g states the formats and the
// two places where this file DEFINES what the reference leaves to the platform (tie order, max == min).  Five entry points:
//
//   v3a_splat_export_filter           rows whose values are all finite (and, on request, whose sigmoid(logit) exceeds a threshold),
//                                     compacted in their original order: a flag per row, an integer scan over blocks of 256, one scatter.
//                                     No atomics.  The survivor count stays on the device; the host reads it once to size the file.
//   v3a_splat_export_sort             Morton order of the survivors (sort_centers, :56-85): per-axis range of their means (partials per
//                                     workgroup, min / max only: order-free), a 30-bit key, rocPRIM radix_sort_pairs - stable, so equal
//                                     keys keep ascending original index.  The one library call in this file.
//   v3a_splat_export_pack_compressed  one workgroup per chunk of 256 sorted splats: its 18 bounds, one 16-byte store per splat, and the
//                                     chunk's 256 x 3K harmonics bytes as whole dwords written by the workgroup together.
//   v3a_splat_export_pack_splat       32 bytes per sorted splat, two 16-byte stores.
//   v3a_splat_export_pack_ply         the surviving rows as interleaved floats, one thread per float (coalesced stores).
//
// Every product-then-sum of the reference is two rounded fp32 operations and every division an IEEE division: contraction is off
// for the whole file, and the divisions are spelled __fdiv_rn.  expf / sqrtf are the device library's (within 1 ulp).
#include "common.h"
#include "int_scan.h"
#include "splat_scene.h"
#include "../../include/vist3a_hip.h"
#include <rocprim/device/device_radix_sort.hpp>

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = 256;             // splats per chunk of the compressed PLY = lanes per workgroup
constexpr int RANGE_BLOCKS = 256;      // at most this many partial ranges: one workgroup of the key kernel reduces them

typedef SplatView<const float> Scene;

__device__ __forceinline__ float sigmoid32(float x) { return __fdiv_rn(1.0f, 1.0f + expf(-x)); }
__device__ __forceinline__ float dc_colour(float sh0) { return sh0 * SH_C0 + 0.5f; }   // sh2rgb: a product, then a sum

// the quaternion of row r in the file's order (w, x, y, z)
__device__ __forceinline__ void load_quat(const Scene& s, long r, float* q) {
  const float* p = s.quats(r);
  if (s.xyzw) { q[0] = p[3]; q[1] = p[0]; q[2] = p[1]; q[3] = p[2]; }
  else { q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = p[3]; }
}
__device__ __forceinline__ float quat_norm(const float* q) { return sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]); }

// ------------------------------------------------------------------------------------------------------------------ filter

struct FilterP {
  Scene s;
  int by_opacity; float threshold;
  unsigned char* flag; int* block_tot; long nb;
  int* rows; long* count;
};

// a flag per row and the flags' total per block of 256 rows.  The harmonics rows of the block are walked by the workgroup together
// (consecutive lanes on consecutive floats); a lane that meets a non-finite value marks the row in LDS (every writer stores the same 1).
__global__ void __launch_bounds__(THREADS) export_flags_kernel(const FilterP a) {
  __shared__ int bad[THREADS];
  __shared__ int buf[THREADS];
  const Scene& s = a.s;
  const long row0 = (long)blockIdx.x * THREADS, g = row0 + threadIdx.x;
  bad[threadIdx.x] = 0;
  __syncthreads();
  const int W = 3 * (s.K + 1);
  const long rows_here = s.rows - row0 < THREADS ? s.rows - row0 : THREADS;
  for (long e = threadIdx.x; e < rows_here * W; e += THREADS) {
    const int r = (int)(e / W), c = (int)(e - (long)r * W);
    if (!finite32(s.sh(row0 + r)[c])) bad[r] = 1;
  }
  __syncthreads();
  int keep = 0;
  if (g < s.rows) {
    bool ok = !bad[threadIdx.x];
#pragma unroll
    for (int e = 0; e < 3; ++e) ok = ok && finite32(s.means(g)[e]) && finite32(s.ls(g)[e]);
#pragma unroll
    for (int e = 0; e < 4; ++e) ok = ok && finite32(s.quats(g)[e]);
    const float logit = s.logit(g);
    ok = ok && finite32(logit);
    if (a.by_opacity) ok = ok && sigmoid32(logit) > a.threshold;
    keep = ok ? 1 : 0;
    a.flag[g] = (unsigned char)keep;
  }
  int total;
  block_exclusive_scan<THREADS>(keep, buf, total);
  if (threadIdx.x == 0) a.block_tot[blockIdx.x] = total;
}

// one workgroup: block_tot becomes its exclusive prefix; *count = the sum
__global__ void __launch_bounds__(THREADS) export_block_prefix_kernel(const FilterP a) {
  __shared__ int buf[THREADS];
  const long run = block_totals_to_prefix<THREADS>(a.block_tot, a.nb, buf);
  if (threadIdx.x == 0) *a.count = run;
}

__global__ void __launch_bounds__(THREADS) export_scatter_kernel(const FilterP a) {
  __shared__ int buf[THREADS];
  const long g = (long)blockIdx.x * THREADS + threadIdx.x;
  const int keep = g < a.s.rows ? a.flag[g] : 0;
  int total;
  const int ex = block_exclusive_scan<THREADS>(keep, buf, total);
  if (keep) a.rows[a.block_tot[blockIdx.x] + ex] = (int)g;
}

// -------------------------------------------------------------------------------------------------------------------- sort

__device__ __forceinline__ float wave_min(float v) { return -wave_max(-v); }   // negation is exact

// min / max of v over the workgroup into every lane (a wave reduction, then four LDS slots); red holds [4][2]
__device__ __forceinline__ void block_min_max(float& lo, float& hi, float (*red)[2]) {
  lo = wave_min(lo);
  hi = wave_max(hi);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[wave][0] = lo; red[wave][1] = hi; }
  __syncthreads();
  lo = fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0]));
  hi = fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1]));
  __syncthreads();
}

struct SortP {
  Scene s;
  const int* rows; long n;
  float* part; int nparts;       // [nparts][6]: min xyz, max xyz of a workgroup's share of the survivors
  unsigned int* key;
};

__global__ void __launch_bounds__(THREADS) export_range_kernel(const SortP a) {
  __shared__ float red[4][2];
  const float inf = __uint_as_float(0x7f800000u);
  float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
  for (long i = (long)blockIdx.x * THREADS + threadIdx.x; i < a.n; i += (long)gridDim.x * THREADS) {
    const float* m = a.s.means(a.rows[i]);
#pragma unroll
    for (int e = 0; e < 3; ++e) { lo[e] = fminf(lo[e], m[e]); hi[e] = fmaxf(hi[e], m[e]); }
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    block_min_max(lo[e], hi[e], red);
    if (threadIdx.x == 0) { a.part[blockIdx.x * 6 + e] = lo[e]; a.part[blockIdx.x * 6 + 3 + e] = hi[e]; }
  }
}

__device__ __forceinline__ unsigned int part1by2(unsigned int x) {
  x &= 0x000003ffu;
  x = (x ^ (x << 16)) & 0xff0000ffu;
  x = (x ^ (x << 8)) & 0x0300f00fu;
  x = (x ^ (x << 4)) & 0x030c30c3u;
  x = (x ^ (x << 2)) & 0x09249249u;
  return x;
}

// every workgroup reduces the (at most 256) partial ranges again, then keys its 256 survivors:
// floor((c - min) / len * 1024) -> int32, & 0x3ff per axis (the maximum's 1024 becomes 0, as in the reference), z highest
__global__ void __launch_bounds__(THREADS) export_keys_kernel(const SortP a) {
  __shared__ float red[4][2];
  const float inf = __uint_as_float(0x7f800000u);
  float mn[3], len[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    float lo = (int)threadIdx.x < a.nparts ? a.part[threadIdx.x * 6 + e] : inf;
    float hi = (int)threadIdx.x < a.nparts ? a.part[threadIdx.x * 6 + 3 + e] : -inf;
    block_min_max(lo, hi, red);
    mn[e] = lo;
    len[e] = hi - lo;
    if (len[e] == 0.f) len[e] = 1.f;
  }
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.n) return;
  const float* m = a.s.means(a.rows[i]);
  unsigned int q[3];
#pragma unroll
  for (int e = 0; e < 3; ++e) q[e] = (unsigned int)(int)floorf(__fdiv_rn(m[e] - mn[e], len[e]) * 1024.f);
  a.key[i] = (part1by2(q[2]) << 2) + (part1by2(q[1]) << 1) + part1by2(q[0]);
}

struct SortLayout { size_t part, key_in, key_out, tmp, tmp_bytes, total; };
SortLayout sort_layout(long U) {
  SortLayout l{};
  size_t off = 0;
  auto take = [&](size_t b) { size_t o = off; off += align256(b); return o; };
  l.part = take(RANGE_BLOCKS * 6 * sizeof(float));
  l.key_in = take((size_t)U * 4);
  l.key_out = take((size_t)U * 4);
  (void)rocprim::radix_sort_pairs(nullptr, l.tmp_bytes, (unsigned int*)nullptr, (unsigned int*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)U, 0, 30);
  l.tmp = take(l.tmp_bytes);
  l.total = off;
  return l;
}

// -------------------------------------------------------------------------------------------------------------------- pack

// pack_unorm: clamp(floor(v t + 0.5), 0, t).  A NaN (0 / 0 where a chunk's max == min) is DEFINED as 0 here.
__device__ __forceinline__ unsigned int unorm(float v, float t) {
  const float f = floorf(v * t + 0.5f);
  return !(f > 0.f) ? 0u : (f >= t ? (unsigned int)t : (unsigned int)f);
}
__device__ __forceinline__ unsigned int pack_111011(float x, float y, float z) {
  return (unorm(x, 2047.f) << 21) | (unorm(y, 1023.f) << 11) | unorm(z, 2047.f);
}
// clamp(v, 0, 255) truncated to a byte (a NaN cannot arrive: the filter has removed it)
__device__ __forceinline__ unsigned int byte_trunc(float v) { return (unsigned int)fminf(fmaxf(v, 0.f), 255.f); }

struct PackP {
  Scene s;
  const int* order; long n;
  float* chunks; u32x4* vertices; unsigned char* shbytes;   // compressed
  u32x4* splat;                                             // .splat
  float* ply;                                               // ply
};

__global__ void __launch_bounds__(THREADS) export_compressed_kernel(const PackP a) {
  __shared__ float red[4][18];
  __shared__ int ord[CHUNK];
  const Scene& s = a.s;
  const int t = threadIdx.x;
  const long first = (long)blockIdx.x * CHUNK, i = first + t;
  const int m = (int)(a.n - first < CHUNK ? a.n - first : CHUNK);     // splats of this chunk
  const bool valid = t < m;
  const long r = a.order[valid ? i : first];     // lanes past the end repeat the chunk's first splat: the bounds do not move
  ord[t] = (int)r;
  float v[9];
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    v[e] = s.means(r)[e];
    v[3 + e] = s.ls(r)[e];
    v[6 + e] = dc_colour(s.sh(r)[(long)e * (s.K + 1)]);
  }
  float lo[9], hi[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) { lo[e] = wave_min(v[e]); hi[e] = wave_max(v[e]); }
  const int wave = t >> 6;
  if ((t & 63) == 0) {
#pragma unroll
    for (int e = 0; e < 9; ++e) { red[wave][e] = lo[e]; red[wave][9 + e] = hi[e]; }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    lo[e] = fminf(fminf(red[0][e], red[1][e]), fminf(red[2][e], red[3][e]));
    hi[e] = fmaxf(fmaxf(red[0][9 + e], red[1][9 + e]), fmaxf(red[2][9 + e], red[3][9 + e]));
  }
#pragma unroll
  for (int e = 3; e < 6; ++e) {     // the log-scale bounds are clamped AFTER the min / max; the values are not
    lo[e] = fminf(fmaxf(lo[e], -20.f), 20.f);
    hi[e] = fminf(fmaxf(hi[e], -20.f), 20.f);
  }
  if (t < 18) {     // min xyz, max xyz, min scale, max scale, min rgb, max rgb
    const int grp = t / 6, w = t % 6, e = grp * 3 + w % 3;
    float b = lo[0];
#pragma unroll
    for (int k = 0; k < 9; ++k) if (k == e) b = w < 3 ? lo[k] : hi[k];
    a.chunks[(long)blockIdx.x * 18 + t] = b;
  }
  if (valid) {
    float nrm[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) nrm[e] = __fdiv_rn(v[e] - lo[e], hi[e] - lo[e]);
    float q[4];
    load_quat(s, r, q);
    const float qn = quat_norm(q);
#pragma unroll
    for (int e = 0; e < 4; ++e) q[e] = __fdiv_rn(q[e], qn);
    int big = 0;
    float qb = q[0];
#pragma unroll
    for (int e = 1; e < 4; ++e)
      if (fabsf(q[e]) > fabsf(qb)) { big = e; qb = q[e]; }     // lowest index on ties
    const float sgn = qb < 0.f ? -1.f : 1.f;
    unsigned int rot = (unsigned int)big << 30;
    int slot = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e == big) continue;
      rot |= unorm((q[e] * sgn) * 0.70710678118654752f + 0.5f, 1023.f) << (20 - 10 * slot);
      ++slot;
    }
    const float op = sigmoid32(s.logit(r));
    u32x4 o;
    o[0] = pack_111011(nrm[0], nrm[1], nrm[2]);
    o[1] = rot;
    o[2] = pack_111011(nrm[3], nrm[4], nrm[5]);
    o[3] = (unorm(nrm[6], 255.f) << 24) | (unorm(nrm[7], 255.f) << 16) | (unorm(nrm[8], 255.f) << 8) | unorm(op, 255.f);
    a.vertices[i] = o;
  }
  // the chunk's harmonics bytes: byte b of the chunk is coefficient j = b % 3K (= c K + k -> sh[c][1 + k]) of its splat b / 3K
  const int K = s.K, W3 = 3 * K;
  if (W3 == 0) return;
  const long nbytes = (long)m * W3;
  unsigned char* dst = a.shbytes + first * W3;
  for (long d = t; 4 * d < nbytes; d += THREADS) {
    const long b0 = 4 * d;
    int sp = (int)(b0 / W3), j = (int)(b0 - (long)sp * W3);
    unsigned int word = 0;
    const int cnt = (int)(nbytes - b0 < 4 ? nbytes - b0 : 4);
    for (int k4 = 0; k4 < cnt; ++k4) {
      const int c = j / K, k = j - c * K;
      const float x = s.sh(ord[sp])[(long)c * (K + 1) + 1 + k];
      word |= byte_trunc(truncf((x * 0.125f + 0.5f) * 256.f)) << (8 * k4);     // x * 0.125 == x / 8 bit for bit
      if (++j == W3) { j = 0; ++sp; }
    }
    if (cnt == 4) *(unsigned int*)(dst + b0) = word;
    else for (int k4 = 0; k4 < cnt; ++k4) dst[b0 + k4] = (unsigned char)(word >> (8 * k4));
  }
}

__global__ void __launch_bounds__(THREADS) export_splat_kernel(const PackP a) {
  const Scene& s = a.s;
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= a.n) return;
  const long r = a.order[i];
  float q[4];
  load_quat(s, r, q);
  const float qn = quat_norm(q);
  unsigned int rot = 0, col = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) rot |= byte_trunc(__fdiv_rn(q[e], qn) * 128.f + 128.f) << (8 * e);
#pragma unroll
  for (int e = 0; e < 3; ++e) col |= byte_trunc(dc_colour(s.sh(r)[(long)e * (s.K + 1)]) * 255.f) << (8 * e);
  col |= byte_trunc(sigmoid32(s.logit(r)) * 255.f) << 24;
  u32x4 o0, o1;
#pragma unroll
  for (int e = 0; e < 3; ++e) o0[e] = __float_as_uint(s.means(r)[e]);
  o0[3] = __float_as_uint(expf(s.ls(r)[0]));
  o1[0] = __float_as_uint(expf(s.ls(r)[1]));
  o1[1] = __float_as_uint(expf(s.ls(r)[2]));
  o1[2] = col;
  o1[3] = rot;
  a.splat[2 * i] = o0;
  a.splat[2 * i + 1] = o1;
}

// x y z, f_dc_0..2, f_rest_0..3K-1, opacity (logit), scale_0..2 (log), rot_0..3 (w x y z)
__global__ void __launch_bounds__(THREADS) export_ply_kernel(const PackP a) {
  const Scene& s = a.s;
  const int K = s.K, Wo = 14 + 3 * K;
  const long e = (long)blockIdx.x * THREADS + threadIdx.x;
  if (e >= a.n * Wo) return;
  const long i = e / Wo;
  const int c = (int)(e - i * Wo);
  const long r = a.order[i];
  float v;
  if (c < 3) v = s.means(r)[c];
  else if (c < 6) v = s.sh(r)[(long)(c - 3) * (K + 1)];
  else if (c < 6 + 3 * K) { const int j = c - 6, ch = j / K; v = s.sh(r)[(long)ch * (K + 1) + 1 + (j - ch * K)]; }
  else if (c == 6 + 3 * K) v = s.logit(r);
  else if (c < 10 + 3 * K) v = s.ls(r)[c - 7 - 3 * K];
  else { const int w = c - 10 - 3 * K; v = s.quats(r)[s.quat_slot(w)]; }
  a.ply[e] = v;
}

// the scene part of the arguments: V3A_OK, or the error code
int scene_of(const v3a_splat_export_args* a, Scene& s) {
  if (!a) return V3A_ERR_ARG;
  if (a->K > 1024) return V3A_ERR_SHAPE;
  return splat_view_of(a, a->U, a->K, s);
}

// the survivor list of a sort / pack call
int list_of(const v3a_splat_export_args* a, const int* list) {
  if (a->n < 0 || a->n > a->U) return V3A_ERR_SHAPE;
  if (a->n > 0 && !list) return V3A_ERR_ARG;
  return V3A_OK;
}

}  // namespace

extern "C" long v3a_splat_export_filter_workspace_bytes(long U, int K) {
  if (bad_count(U) || K < 0 || K > 1024) return V3A_ERR_SHAPE;
  return (long)(align256((size_t)U) + align256((size_t)scan_blocks<THREADS>(U) * sizeof(int)));
}

extern "C" int v3a_splat_export_filter(const v3a_splat_export_args* a, void* stream_) {
  FilterP k{};
  const int rc = scene_of(a, k.s);
  if (rc != V3A_OK) return rc;
  if (!a->count) return V3A_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  if (a->U == 0) return hipMemsetAsync(a->count, 0, sizeof(long), stream) == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
  if (!a->rows) return V3A_ERR_ARG;
  if (bad_workspace(a->workspace, a->workspace_bytes, v3a_splat_export_filter_workspace_bytes(a->U, a->K))) return V3A_ERR_WORKSPACE;
  k.by_opacity = a->filter_opacity != 0; k.threshold = a->opacity_threshold;
  k.flag = (unsigned char*)a->workspace;
  k.block_tot = (int*)((char*)a->workspace + align256((size_t)a->U));
  k.nb = scan_blocks<THREADS>(a->U);
  k.rows = a->rows; k.count = a->count;
  hipLaunchKernelGGL(export_flags_kernel, dim3((unsigned)k.nb), dim3(THREADS), 0, stream, k);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(export_block_prefix_kernel, dim3(1), dim3(THREADS), 0, stream, k);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(export_scatter_kernel, dim3((unsigned)k.nb), dim3(THREADS), 0, stream, k);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" long v3a_splat_export_sort_workspace_bytes(long U, int K) {
  if (bad_count(U) || K < 0 || K > 1024) return V3A_ERR_SHAPE;
  return (long)sort_layout(U).total;
}

extern "C" int v3a_splat_export_sort(const v3a_splat_export_args* a, void* stream_) {
  SortP k{};
  int rc = scene_of(a, k.s);
  if (rc != V3A_OK) return rc;
  if ((rc = list_of(a, a->rows)) != V3A_OK) return rc;
  if (a->n == 0) return V3A_OK;
  if (!a->order) return V3A_ERR_ARG;
  const SortLayout l = sort_layout(a->U);
  if (bad_workspace(a->workspace, a->workspace_bytes, (long)l.total)) return V3A_ERR_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)a->workspace;
  k.rows = a->rows; k.n = a->n;
  k.part = (float*)(ws + l.part);
  const long nb = blocks_for(a->n, THREADS);
  k.nparts = (int)(nb < RANGE_BLOCKS ? nb : RANGE_BLOCKS);
  k.key = (unsigned int*)(ws + l.key_in);
  hipLaunchKernelGGL(export_range_kernel, dim3((unsigned)k.nparts), dim3(THREADS), 0, stream, k);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(export_keys_kernel, dim3((unsigned)nb), dim3(THREADS), 0, stream, k);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  size_t tb = 0;     // what the sort wants for n items: never more than the workspace holds for U
  (void)rocprim::radix_sort_pairs(nullptr, tb, (unsigned int*)nullptr, (unsigned int*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)a->n, 0, 30);
  if (tb > l.tmp_bytes) return V3A_ERR_WORKSPACE;
  tb = l.tmp_bytes;
  if (rocprim::radix_sort_pairs(ws + l.tmp, tb, k.key, (unsigned int*)(ws + l.key_out), a->rows, a->order, (size_t)a->n, 0, 30, stream) != hipSuccess)
    return V3A_ERR_LAUNCH;
  return V3A_OK;
}

extern "C" int v3a_splat_export_pack_compressed(const v3a_splat_export_args* a, void* stream) {
  PackP k{};
  int rc = scene_of(a, k.s);
  if (rc != V3A_OK) return rc;
  if ((rc = list_of(a, a->order)) != V3A_OK) return rc;
  if (a->n == 0) return V3A_OK;
  if (!a->out_chunks || !a->out_vertices || (a->K > 0 && !a->out_sh)) return V3A_ERR_ARG;
  if (((uintptr_t)a->out_chunks & 3) || ((uintptr_t)a->out_vertices & 15) || ((uintptr_t)a->out_sh & 3)) return V3A_ERR_SHAPE;
  k.order = a->order; k.n = a->n;
  k.chunks = a->out_chunks; k.vertices = (u32x4*)a->out_vertices; k.shbytes = a->out_sh;
  hipLaunchKernelGGL(export_compressed_kernel, dim3(blocks_for(a->n, CHUNK)), dim3(THREADS), 0, (hipStream_t)stream, k);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_splat_export_pack_splat(const v3a_splat_export_args* a, void* stream) {
  PackP k{};
  int rc = scene_of(a, k.s);
  if (rc != V3A_OK) return rc;
  if ((rc = list_of(a, a->order)) != V3A_OK) return rc;
  if (a->n == 0) return V3A_OK;
  if (!a->out_splat) return V3A_ERR_ARG;
  if ((uintptr_t)a->out_splat & 15) return V3A_ERR_SHAPE;
  k.order = a->order; k.n = a->n;
  k.splat = (u32x4*)a->out_splat;
  hipLaunchKernelGGL(export_splat_kernel, dim3(blocks_for(a->n, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, k);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_splat_export_pack_ply(const v3a_splat_export_args* a, void* stream) {
  PackP k{};
  int rc = scene_of(a, k.s);
  if (rc != V3A_OK) return rc;
  if ((rc = list_of(a, a->rows)) != V3A_OK) return rc;
  if (a->n == 0) return V3A_OK;
  if (!a->out_ply) return V3A_ERR_ARG;
  const long total = a->n * (14 + 3L * a->K);
  if (((uintptr_t)a->out_ply & 3) || blocks_for(total, THREADS) > 0x7fffffffL) return V3A_ERR_SHAPE;
  k.order = a->rows; k.n = a->n;
  k.ply = a->out_ply;
  hipLaunchKernelGGL(export_ply_kernel, dim3(blocks_for(total, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, k);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
