// Scene import decoded on the device: the float PLY, the compressed PLY (SuperSplat) and the 32-byte .splat (antimatter15) that
// splat_export.hip writes - or any other trainer's standard 3DGS PLY - read back into the trainer's storage (means, log-scales,
// quaternions, opacity logits, harmonics [n,3,K+1]).  DESIGN.md section 7h states the decoding.  Three entry points:
//
//   v3a_splat_import_ply         a workgroup walks the floats of 256 consecutive rows in file order (consecutive lanes on consecutive
//                                floats: the file is read once, coalesced); a column table in LDS says where a float goes.  Row and
//                                column of a lane advance by a fixed step: no division per element.
//   v3a_splat_import_compressed  one workgroup per chunk of 256 splats, one lane per splat - the mirror of the pack kernel.  The
//                                chunk's 18 bounds are read once into LDS; the chunk's harmonics bytes are walked by the workgroup
//                                together.  Vertex words are read as single dwords and harmonics as single bytes: the vertex
//                                section starts 72 x chunks into the payload and a splat's 3K bytes may be an odd count.
//   v3a_splat_import_splat       one lane per 32-byte record.
//
// Every output element is written exactly once with plain stores.  `bad`, the number of rows with a non-finite output: a flag per
// row, block_sum (fixed_sum.h) per workgroup into the workspace, and one workgroup that adds the totals (int_scan.h).  Integers:
// no order can change it.  No memset, no atomics.
//
// Every product-then-sum is two rounded fp32 operations and every division an IEEE division: contraction is off for the whole
// file and the divisions are spelled __fdiv_rn.  logf / sqrtf are the device library's (within 1 ulp).
#include "common.h"
#include "fixed_sum.h"
#include "int_scan.h"
#include "splat_scene.h"
#include "../../include/vist3a_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int CHUNK = 256;             // splats per chunk of the compressed PLY = lanes per workgroup
constexpr int MAX_P = 4096;            // floats per row of a float PLY: the column table is LDS
constexpr int MAX_K = 63;
constexpr float SQRT2 = 1.4142135623730951f;

typedef SplatView<float> Out;

// the logit of an opacity code c in (0, 255): exact operands, one division, one logf
__device__ __forceinline__ float logit_of_code(float c) { return logf(__fdiv_rn(c, 255.f - c)); }
__device__ __forceinline__ float unlerp(float lo, float hi, unsigned int code, float top) { return lo + (hi - lo) * __fdiv_rn((float)code, top); }

// the workgroup's number of flagged rows into its slot of the totals.  All lanes must call it.
__device__ __forceinline__ void store_block_total(int flag, int* red, int* block_tot) {
  const int total = block_sum<THREADS>(flag, red);
  if (threadIdx.x == 0) block_tot[blockIdx.x] = total;
}

// one workgroup: *bad = the sum of the workgroups' totals
__global__ void __launch_bounds__(THREADS) import_bad_total_kernel(int* block_tot, long nb, int* bad) {
  __shared__ int buf[THREADS];
  const long run = block_totals_to_prefix<THREADS>(block_tot, nb, buf);
  if (threadIdx.x == 0) *bad = (int)run;
}

// --------------------------------------------------------------------------------------------------------------- float PLY

struct PlyP {
  Out o;
  const float* in;
  int P, n_rest, linear;
  int off[15];       // x y z, f_dc_0..2, f_rest_0, opacity, scale_0..2, rot_0..3
  int* block_tot;
};

__global__ void __launch_bounds__(THREADS) import_ply_kernel(const PlyP a) {
  __shared__ int lut[MAX_P];       // column -> (tensor << 16) | element of the row, or -1: not ours
  __shared__ int bad[THREADS];
  __shared__ int red[THREADS];
  const Out& o = a.o;
  const int t = threadIdx.x, P = a.P, K = o.K;
  for (int c = t; c < P; c += THREADS) lut[c] = -1;
  bad[t] = 0;
  __syncthreads();
  if (t < 15 && t != 6) {
    int col = a.off[0];
#pragma unroll
    for (int k = 1; k < 15; ++k) if (t == k) col = a.off[k];
    int code;
    if (t < 3) code = (SPLAT_MEANS << 16) | t;
    else if (t < 6) code = (SPLAT_SH << 16) | ((t - 3) * (K + 1));
    else if (t == 7) code = SPLAT_LOGITS << 16;
    else if (t < 11) code = (SPLAT_LS << 16) | (t - 8);
    else code = (SPLAT_QUATS << 16) | o.quat_slot(t - 11);
    lut[col] = code;
  }
  for (int j = t; j < a.n_rest; j += THREADS) {
    const int c = j / K, k = j - c * K;
    lut[a.off[6] + j] = (SPLAT_SH << 16) | (c * (K + 1) + 1 + k);
  }
  __syncthreads();
  const long row0 = (long)blockIdx.x * THREADS;
  const int rows_here = (int)(o.rows - row0 < THREADS ? o.rows - row0 : THREADS);
  const int total = rows_here * P;                       // <= 256 * 4096
  const float* src = a.in + row0 * P;
  const int dq = THREADS / P, dr = THREADS - dq * P;     // a lane's step of 256 floats = dq rows and dr columns
  int r = t / P, c = t - r * P;
  const float hi = (float)(1.0 - 1e-6);
  for (int e = t; e < total; e += THREADS) {
    const int code = lut[c];
    if (code >= 0) {
      float v = src[e];
      const int kind = code >> 16, idx = code & 0xffff;
      if (kind == SPLAT_LOGITS && a.linear) {
        v = v < 1e-6f ? 1e-6f : (v > hi ? hi : v);       // a NaN stays a NaN
        v = logf(__fdiv_rn(v, 1.f - v));
      }
      // o.p[kind] spelled as selects: the view stays in scalar registers
      float* base = kind == SPLAT_MEANS ? o.p[SPLAT_MEANS] : kind == SPLAT_LS ? o.p[SPLAT_LS] : kind == SPLAT_QUATS ? o.p[SPLAT_QUATS] : kind == SPLAT_LOGITS ? o.p[SPLAT_LOGITS] : o.p[SPLAT_SH];
      const long ld = kind == SPLAT_MEANS ? o.ld[SPLAT_MEANS] : kind == SPLAT_LS ? o.ld[SPLAT_LS] : kind == SPLAT_QUATS ? o.ld[SPLAT_QUATS] : kind == SPLAT_LOGITS ? o.ld[SPLAT_LOGITS] : o.ld[SPLAT_SH];
      base[(row0 + r) * ld + idx] = v;
      if (!finite32(v)) bad[r] = 1;                      // every writer stores the same 1
    }
    c += dr;
    r += dq;
    if (c >= P) { c -= P; ++r; }
  }
  __syncthreads();
  store_block_total(t < rows_here ? bad[t] : 0, red, a.block_tot);
}

// ---------------------------------------------------------------------------------------------------------- compressed PLY

struct CompP {
  Out o;
  const float* chunks; const unsigned int* vertices; const unsigned char* shbytes;
  int* block_tot;
};

__global__ void __launch_bounds__(THREADS) import_compressed_kernel(const CompP a) {
  __shared__ float bnd[18];          // min xyz, max xyz, min scale, max scale, min rgb, max rgb
  __shared__ int col[3 * MAX_K];     // f_rest_j -> its element of the harmonics row
  __shared__ int red[THREADS];
  const Out& o = a.o;
  const int t = threadIdx.x, K = o.K, W3 = 3 * K;
  const long first = (long)blockIdx.x * CHUNK, i = first + t;
  const int m = (int)(o.rows - first < CHUNK ? o.rows - first : CHUNK);     // splats of this chunk
  if (t < 18) bnd[t] = a.chunks[(long)blockIdx.x * 18 + t];
  if (t < W3) { const int c = t / K; col[t] = c * (K + 1) + 1 + (t - c * K); }
  __syncthreads();
  int flag = 0;
  if (t < m) {
    const unsigned int* w = a.vertices + 4 * i;
    const unsigned int pos = w[0], rot = w[1], scl = w[2], rgba = w[3];
    const unsigned int pc[3] = {pos >> 21, (pos >> 11) & 1023u, pos & 2047u}, sc[3] = {scl >> 21, (scl >> 11) & 1023u, scl & 2047u};
    const unsigned int cc[3] = {rgba >> 24, (rgba >> 16) & 255u, (rgba >> 8) & 255u};
    const float top[3] = {2047.f, 1023.f, 2047.f};
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const float mean = unlerp(bnd[e], bnd[3 + e], pc[e], top[e]);
      const float ls = unlerp(bnd[6 + e], bnd[9 + e], sc[e], top[e]);
      const float sh0 = __fdiv_rn(unlerp(bnd[12 + e], bnd[15 + e], cc[e], 255.f) - 0.5f, SH_C0);
      o.means(i)[e] = mean;
      o.ls(i)[e] = ls;
      o.sh(i)[(long)e * (K + 1)] = sh0;
      ok = ok && finite32(mean) && finite32(ls) && finite32(sh0);
    }
    flag = ok ? 0 : 1;                                   // the logit and the quaternion of a code are always finite
    const float c = fminf(fmaxf((float)(rgba & 255u), 0.5f), 254.5f);
    o.logit(i) = logit_of_code(c);
    float v[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) v[e] = (__fdiv_rn((float)((rot >> (20 - 10 * e)) & 1023u), 1023.f) - 0.5f) * SQRT2;
    const float dropped = sqrtf(fmaxf(0.f, 1.f - ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])));
    const int big = (int)(rot >> 30);
#pragma unroll
    for (int e = 0; e < 4; ++e) {                        // the stored three fill the other places in ascending order
      const int slot = e - (e > big ? 1 : 0);
      const float q = e == big ? dropped : (slot == 0 ? v[0] : slot == 1 ? v[1] : v[2]);
      o.quats(i)[o.quat_slot(e)] = q;
    }
  }
  // the chunk's harmonics bytes: byte b of the chunk is coefficient j = b % 3K of its splat b / 3K; a lane's step of 256 bytes is
  // dq splats and dr coefficients
  if (W3 > 0) {
    const unsigned char* src = a.shbytes + first * W3;
    const int nbytes = m * W3;
    const int dq = THREADS / W3, dr = THREADS - dq * W3;
    int sp = t / W3, j = t - sp * W3;
    for (int e = t; e < nbytes; e += THREADS) {
      const float x = (((float)src[e] + 0.5f) * 0.00390625f - 0.5f) * 8.f;     // * 2^-8 == / 256 bit for bit
      o.sh(first + sp)[col[j]] = x;
      j += dr;
      sp += dq;
      if (j >= W3) { j -= W3; ++sp; }
    }
  }
  store_block_total(flag, red, a.block_tot);
}

// ------------------------------------------------------------------------------------------------------------------ .splat

struct SplatP {
  Out o;
  const unsigned int* in;       // 8 dwords per splat
  int* block_tot;
};

__global__ void __launch_bounds__(THREADS) import_splat_kernel(const SplatP a) {
  __shared__ int red[THREADS];
  const Out& o = a.o;
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  int flag = 0;
  if (i < o.rows) {
    unsigned int w[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = a.in[8 * i + e];
    bool ok = true;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const float mean = __uint_as_float(w[e]);
      const float ls = logf(__uint_as_float(w[3 + e]));   // a scale <= 0, NaN or Inf leaves a non-finite log: the row is bad
      const float rgb = __fdiv_rn((float)((w[6] >> (8 * e)) & 255u) + 0.5f, 255.f);
      o.means(i)[e] = mean;
      o.ls(i)[e] = ls;
      o.sh(i)[e] = __fdiv_rn(rgb - 0.5f, SH_C0);
      ok = ok && finite32(mean) && finite32(ls);
    }
    flag = ok ? 0 : 1;
    o.logit(i) = logit_of_code(fminf(fmaxf((float)(w[6] >> 24) + 0.5f, 0.5f), 254.5f));
#pragma unroll
    for (int e = 0; e < 4; ++e)
      o.quats(i)[o.quat_slot(e)] = ((float)((w[7] >> (8 * e)) & 255u) + 0.5f - 128.f) * 0.0078125f;   // / 128, exact
  }
  store_block_total(flag, red, a.block_tot);
}

// --------------------------------------------------------------------------------------------------------------- host side

// the output part of the arguments: V3A_OK, with o.rows > 0 when there is something to launch, or the error code
int out_of(const v3a_splat_import_args* a, Out& o) {
  if (!a) return V3A_ERR_ARG;
  if (bad_count(a->n) || a->n_rest < 0 || a->n_rest % 3 != 0 || a->n_rest / 3 > MAX_K) return V3A_ERR_SHAPE;
  if (a->n > 0 && (!a->bad || !a->payload)) return V3A_ERR_ARG;
  const int rc = splat_view_of(a, a->n, a->n_rest / 3, o);
  if (rc == V3A_OK && a->n > 0 && ((uintptr_t)a->payload & 3)) return V3A_ERR_SHAPE;
  return rc;
}

int workspace_of(const v3a_splat_import_args* a) {
  return bad_workspace(a->workspace, a->workspace_bytes, v3a_splat_import_workspace_bytes(a->n)) ? V3A_ERR_WORKSPACE : V3A_OK;
}

int finish(const v3a_splat_import_args* a, hipStream_t stream) {
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(import_bad_total_kernel, dim3(1), dim3(THREADS), 0, stream, (int*)a->workspace, blocks_for(a->n, THREADS), a->bad);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

}  // namespace

extern "C" long v3a_splat_import_workspace_bytes(long n) {
  if (bad_count(n)) return V3A_ERR_SHAPE;
  return (long)align256((size_t)blocks_for(n, THREADS) * sizeof(int));
}

extern "C" int v3a_splat_import_ply(const v3a_splat_import_args* a, void* stream_) {
  PlyP k{};
  int rc = out_of(a, k.o);
  if (rc != V3A_OK || k.o.rows == 0) return rc;
  const int P = a->P;
  if (P < 14 + a->n_rest || P > MAX_P) return V3A_ERR_SHAPE;
  for (int e = 0; e < 15; ++e) {
    const int width = e == 6 ? a->n_rest : 1;
    if (a->offsets[e] < 0 || a->offsets[e] + width > P) return V3A_ERR_SHAPE;
    for (int f = 0; f < e; ++f) {     // no column twice: every output element has exactly one source
      const int wf = f == 6 ? a->n_rest : 1;
      if (a->offsets[e] < a->offsets[f] + wf && a->offsets[f] < a->offsets[e] + width) return V3A_ERR_SHAPE;
    }
  }
  if (a->payload_bytes != 4L * a->n * P) return V3A_ERR_SHAPE;
  if ((rc = workspace_of(a)) != V3A_OK) return rc;
  k.in = (const float*)a->payload;
  k.P = P; k.n_rest = a->n_rest; k.linear = a->opacity_linear != 0;
  for (int e = 0; e < 15; ++e) k.off[e] = a->offsets[e];
  k.block_tot = (int*)a->workspace;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(import_ply_kernel, dim3((unsigned)blocks_for(a->n, THREADS)), dim3(THREADS), 0, stream, k);
  return finish(a, stream);
}

extern "C" int v3a_splat_import_compressed(const v3a_splat_import_args* a, void* stream_) {
  CompP k{};
  int rc = out_of(a, k.o);
  if (rc != V3A_OK || k.o.rows == 0) return rc;
  if (a->nch != blocks_for(a->n, CHUNK) || a->payload_bytes != 72L * a->nch + 16L * a->n + (long)a->n_rest * a->n) return V3A_ERR_SHAPE;
  if ((rc = workspace_of(a)) != V3A_OK) return rc;
  k.chunks = (const float*)a->payload;
  k.vertices = (const unsigned int*)(a->payload + 72L * a->nch);
  k.shbytes = a->payload + 72L * a->nch + 16L * a->n;
  k.block_tot = (int*)a->workspace;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(import_compressed_kernel, dim3((unsigned)a->nch), dim3(THREADS), 0, stream, k);
  return finish(a, stream);
}

extern "C" int v3a_splat_import_splat(const v3a_splat_import_args* a, void* stream_) {
  SplatP k{};
  int rc = out_of(a, k.o);
  if (rc != V3A_OK || k.o.rows == 0) return rc;
  if (a->n_rest != 0 || a->payload_bytes != 32L * a->n) return V3A_ERR_SHAPE;
  if ((rc = workspace_of(a)) != V3A_OK) return rc;
  k.in = (const unsigned int*)a->payload;
  k.block_tot = (int*)a->workspace;
  hipStream_t stream = (hipStream_t)stream_;
  hipLaunchKernelGGL(import_splat_kernel, dim3((unsigned)blocks_for(a->n, THREADS)), dim3(THREADS), 0, stream, k);
  return finish(a, stream);
}
