// CLIP score of the generated-scene evaluation (evaluation/gen_eval/t3_scene_evaluation.py:97-120 of the reference: torchmetrics CLIPScore
// on a Hugging Face CLIPModel): the passes around the towers' split GEMMs.  The linear layers are v3a_conv_split as 1x1 convolutions
// (fp32-equivalent, QUICK_GELU in the fp32 epilogue), the LayerNorms v3a_layernorm / v3a_layernorm_pair; this file holds
//   1. clip_resize_h_kernel / clip_resize_v_kernel   CLIPImageProcessor on the Pillow path for N uint8 frames [N,H,W,3]: Pillow's BICUBIC
//        (ImagingResample, 8 bits per channel) with the coefficient tables the host computed in float64 and converted to 22-bit fixed
//        point - the kernels do integer work only: clip8(((1 << 21) + sum k_i p_i) >> 22), horizontal pass first, the intermediate rounded
//        to uint8, then the vertical pass.  Only the centre crop's columns (pass 1) and the rows its vertical taps read are computed.  The
//        second pass maps the uint8 result through a host-built table [3][256] (rescale and normalise, fp32, transformers' own roundings)
//        and writes the crop as the patch matrix [N (S / P)^2][ldk] of (hi, lo) bf16 pairs, column = c P^2 + py P + px, columns
//        3 P^2 .. ldk zero: the patch convolution (stride = kernel) is then one split GEMM.  Optional outputs: the uint8 crop [N,S,S,3] and
//        the fp32 pixel values [N,3,S,S].
//   2. clip_rows_kernel        token assembly into the f32 residual stream: out[r] = src[row(r)] + pos[r % S], row(r) = ids[r] (token /
//        EOS-row gather), or the class token at r % S == 0 and patch row r - r / S - 1 elsewhere.
//   3. attention_f32_kernel    softmax(q k^T scale [+ causal mask, keys < len_b]) v for B sequences x H heads of 64 channels, S <= 1024,
//        everything fp32: one query row per lane (q and the output row in registers), 64 query rows per one-wave workgroup, K / V tiles of
//        32 keys in LDS (read as broadcasts: every lane reads the same address), online softmax with one rescale per tile.  A row's keys are
//        visited in index order by one lane: results do not depend on the launch's batch, head count or on other rows.
//   4. clip_score_kernel       fp64: s_f = max(100 <i_f, t> / (|i_f| |t|), 0) for F image embeddings against one text embedding, and
//        their mean summed in frame order.  One workgroup, the reductions of fixed_sum.h, no atomics.
//
// Bounds: the resize passes and the token assembly are streaming passes (bytes); attention_f32 does 2 S^2 64 FMAs
// per head, one lane per row, behind LDS broadcast reads of 16 B per 4 FMAs at one wave per SIMD - LDS / global latency, not the VALU,
// is what most likely bounds it (not measured).
#include "common.h"
#include "fixed_sum.h"
#include "../../include/vist3a_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int PRECISION_BITS = 22;   // Pillow Resample.c: 32 - 8 - 2

__device__ __forceinline__ int clip8(int v) {
  v >>= PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct ResizeP {
  const unsigned char* src;   // [N][H][W][3]
  unsigned char* tmp;         // [N][R][S][3]: rows r0 .. r0 + R of the horizontally resampled image, crop columns only
  const int* xb;              // [S][2]  first input column, tap count
  const int* xk;              // [S][kx] fixed-point coefficients
  const int* yb;              // [S][2]  first input row, tap count
  const int* yk;              // [S][ky]
  const float* lut;           // [3][256]
  char* p_hi;                 // [N G G][ldk] bf16
  char* p_lo;
  unsigned char* out_u8;      // [N][S][S][3] or null
  float* out_f32;             // [N][3][S][S] or null
  int N, H, W, S, P, ldk, kx, ky, r0, R;
};

// one thread = one (frame, kept input row, crop column), 3 channels
__global__ void __launch_bounds__(THREADS) clip_resize_h_kernel(ResizeP p) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  const long total = (long)p.N * p.R * p.S;
  if (i >= total) return;
  const int x = (int)(i % p.S);
  const int r = (int)((i / p.S) % p.R);
  const int n = (int)(i / ((long)p.S * p.R));
  const int x0 = p.xb[2 * x], cnt = p.xb[2 * x + 1];
  const unsigned char* s = p.src + (((size_t)n * p.H + p.r0 + r) * p.W + x0) * 3;
  const int* k = p.xk + (size_t)x * p.kx;
  int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
  for (int t = 0; t < cnt; ++t) {
    const int c = k[t];
    a0 += c * (int)s[3 * t];
    a1 += c * (int)s[3 * t + 1];
    a2 += c * (int)s[3 * t + 2];
  }
  unsigned char* d = p.tmp + (size_t)i * 3;
  d[0] = (unsigned char)clip8(a0);
  d[1] = (unsigned char)clip8(a1);
  d[2] = (unsigned char)clip8(a2);
}

// one thread = one (frame, crop row, crop column), 3 channels: vertical pass, table, split, patch-matrix store
__global__ void __launch_bounds__(THREADS) clip_resize_v_kernel(ResizeP p) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  const long total = (long)p.N * p.S * p.S;
  if (i >= total) return;
  const int x = (int)(i % p.S);
  const int y = (int)((i / p.S) % p.S);
  const int n = (int)(i / ((long)p.S * p.S));
  const int y0 = p.yb[2 * y] - p.r0, cnt = p.yb[2 * y + 1];
  const unsigned char* s = p.tmp + (((size_t)n * p.R + y0) * p.S + x) * 3;
  const size_t pitch = (size_t)p.S * 3;
  const int* k = p.yk + (size_t)y * p.ky;
  int a[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
  for (int t = 0; t < cnt; ++t) {
    const int c = k[t];
    a[0] += c * (int)s[t * pitch];
    a[1] += c * (int)s[t * pitch + 1];
    a[2] += c * (int)s[t * pitch + 2];
  }
  const int G = p.S / p.P, py = y % p.P, px = x % p.P;
  const size_t row = ((size_t)n * G + y / p.P) * G + x / p.P;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int u = clip8(a[c]);
    const float f = p.lut[c * 256 + u];
    const unsigned short h = f32_to_bf16(f);
    const unsigned short l = f32_to_bf16(f - bf16_to_f32(h));   // the difference is exact in fp32
    const size_t o = (row * p.ldk + (size_t)c * p.P * p.P + py * p.P + px) * 2;
    *(unsigned short*)(p.p_hi + o) = h;
    *(unsigned short*)(p.p_lo + o) = l;
    if (p.out_u8) p.out_u8[(size_t)i * 3 + c] = (unsigned char)u;
    if (p.out_f32) p.out_f32[(((size_t)n * 3 + c) * p.S + y) * p.S + x] = f;
  }
  if (py == 0 && px == 0) {   // the padding columns of this patch's row
    for (int c = 3 * p.P * p.P; c < p.ldk; ++c) {
      *(unsigned short*)(p.p_hi + (row * p.ldk + c) * 2) = 0;
      *(unsigned short*)(p.p_lo + (row * p.ldk + c) * 2) = 0;
    }
  }
}

struct RowsP {
  const float* src;
  const int* ids;     // [M] source rows, or null
  const float* cls;   // [d] or null (with ids null: vision assembly)
  const float* pos;   // [S][d] or null
  float* out;         // [M][d]
  long M;
  int S, d, src_rows;
};

// one thread = 4 channels of one output row
__global__ void __launch_bounds__(THREADS) clip_rows_kernel(RowsP p) {
  const long i = (long)blockIdx.x * THREADS + threadIdx.x;
  const int d4 = p.d / 4;
  if (i >= p.M * d4) return;
  const long r = i / d4;
  const int c = (int)(i % d4) * 4;
  const int s = (int)(r % p.S);
  f32x4 v;
  if (p.ids) {
    int id = p.ids[r];
    id = id < 0 ? 0 : (id >= p.src_rows ? p.src_rows - 1 : id);   // validated on the host; never read out of bounds
    v = *(const f32x4*)(p.src + (size_t)id * p.d + c);
  } else if (p.cls) {
    v = s == 0 ? *(const f32x4*)(p.cls + c) : *(const f32x4*)(p.src + (size_t)(r - r / p.S - 1) * p.d + c);
  } else {
    v = *(const f32x4*)(p.src + (size_t)r * p.d + c);
  }
  if (p.pos) {
    const f32x4 q = *(const f32x4*)(p.pos + (size_t)s * p.d + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += q[e];
  }
  *(f32x4*)(p.out + (size_t)r * p.d + c) = v;
}

// ------------------------------------------------------------------------------------------------ fp32 attention, hd = 64
constexpr int HD = 64, QT = 64, KT = 32;

struct AttnP {
  const float* q;
  const float* k;
  const float* v;
  char* o_hi;
  char* o_lo;
  float* o_f32;
  const int* lens;
  int ld, ldo, B, S, H, causal;
  float scale;
};

__global__ void __launch_bounds__(QT) attention_f32_kernel(AttnP p) {
  __shared__ __attribute__((aligned(16))) float Ks[KT][HD];
  __shared__ __attribute__((aligned(16))) float Vs[KT][HD];
  const int lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int q0 = blockIdx.x * QT;
  const int qi = q0 + lane;
  const bool live = qi < p.S;
  int len = p.lens ? p.lens[b] : p.S;
  len = len < 1 ? 1 : (len > p.S ? p.S : len);
  const size_t base = (size_t)b * p.S;
  float qr[HD], acc[HD];
  {
    const float* qp = p.q + (base + (live ? qi : p.S - 1)) * p.ld + h * HD;
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
      const f32x4 t = *(const f32x4*)(qp + c);
      qr[c] = t[0]; qr[c + 1] = t[1]; qr[c + 2] = t[2]; qr[c + 3] = t[3];
    }
  }
#pragma unroll
  for (int c = 0; c < HD; ++c) acc[c] = 0.f;
  float m = -INFINITY, l = 0.f;
  // keys this workgroup needs: below the valid length, and under the causal mask up to its last query row
  int kend = len;
  if (p.causal) kend = min(kend, min(q0 + QT, p.S));
  for (int j0 = 0; j0 < kend; j0 += KT) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < KT * HD / 4 / QT; ++it) {
      const int idx = it * QT + lane;
      const int kr = idx / (HD / 4), c4 = (idx % (HD / 4)) * 4;
      const int j = j0 + kr;
      f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
      if (j < kend) {
        kv = *(const f32x4*)(p.k + (base + j) * p.ld + h * HD + c4);
        vv = *(const f32x4*)(p.v + (base + j) * p.ld + h * HD + c4);
      }
      *(f32x4*)&Ks[kr][c4] = kv;
      *(f32x4*)&Vs[kr][c4] = vv;
    }
    __syncthreads();
    float s[KT];
    float tmax = -INFINITY;
#pragma unroll
    for (int kr = 0; kr < KT; ++kr) {
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < HD; c += 4) {
        const f32x4 t = *(const f32x4*)&Ks[kr][c];
        d = fmaf(qr[c], t[0], d);
        d = fmaf(qr[c + 1], t[1], d);
        d = fmaf(qr[c + 2], t[2], d);
        d = fmaf(qr[c + 3], t[3], d);
      }
      const int j = j0 + kr;
      const bool ok = j < kend && (!p.causal || j <= qi || !live);
      s[kr] = ok ? d * p.scale : -INFINITY;
      tmax = fmaxf(tmax, s[kr]);
    }
    // key j0 is visible to every row of the tile that reaches it (j0 <= q0 under the causal mask): tmax is finite from the first tile on
    const float mn = fmaxf(m, tmax);
    const float alpha = expf(m - mn);   // first tile: exp(-inf) = 0
    l *= alpha;
#pragma unroll
    for (int c = 0; c < HD; ++c) acc[c] *= alpha;
#pragma unroll
    for (int kr = 0; kr < KT; ++kr) {
      const float e = expf(s[kr] - mn);   // masked keys: exp(-inf) = 0
      l += e;
#pragma unroll
      for (int c = 0; c < HD; c += 4) {
        const f32x4 t = *(const f32x4*)&Vs[kr][c];
        acc[c] = fmaf(e, t[0], acc[c]);
        acc[c + 1] = fmaf(e, t[1], acc[c + 1]);
        acc[c + 2] = fmaf(e, t[2], acc[c + 2]);
        acc[c + 3] = fmaf(e, t[3], acc[c + 3]);
      }
    }
    m = mn;
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < HD; ++c) acc[c] = acc[c] / l;
  const size_t o = (base + qi) * p.ldo + h * HD;
  if (p.o_f32) {
#pragma unroll
    for (int c = 0; c < HD; c += 4) {
      const f32x4 t = {acc[c], acc[c + 1], acc[c + 2], acc[c + 3]};
      *(f32x4*)(p.o_f32 + o + c) = t;
    }
  }
  if (p.o_hi) {
#pragma unroll
    for (int c = 0; c < HD; c += 8) {
      const u32x4 hh = pack_bf16x8(acc + c);
      float hf[8], r[8];
      unpack_bf16x8(hh, hf);
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = acc[c + e] - hf[e];   // exact in fp32
      *(u32x4*)(p.o_hi + (o + c) * 2) = hh;
      *(u32x4*)(p.o_lo + (o + c) * 2) = pack_bf16x8(r);
    }
  }
}

// ------------------------------------------------------------------------------------------------ score head (fp64)
__global__ void __launch_bounds__(THREADS) clip_score_kernel(const float* img, const float* txt, int F, int D, double* scores, double* mean) {
  __shared__ double red[THREADS];
  const int tid = threadIdx.x;
  double tt = 0.0;
  for (int c = tid; c < D; c += THREADS) tt += (double)txt[c] * (double)txt[c];
  tt = block_sum<THREADS>(tt, red);
  double total = 0.0;
  for (int f = 0; f < F; ++f) {
    double ii = 0.0, it = 0.0;
    for (int c = tid; c < D; c += THREADS) {
      const double a = (double)img[(size_t)f * D + c];
      ii += a * a;
      it += a * (double)txt[c];
    }
    ii = block_sum<THREADS>(ii, red);
    it = block_sum<THREADS>(it, red);
    double s = 100.0 * (it / (sqrt(ii) * sqrt(tt)));
    s = s < 0.0 ? 0.0 : s;   // torchmetrics: max(score, 0); a NaN (zero embedding) stays NaN, as there
    if (tid == 0) scores[f] = s;
    total += s;
  }
  if (tid == 0 && mean) *mean = total / (double)F;
}

}  // namespace

extern "C" long v3a_clip_preprocess_workspace_bytes(int N, int rows, int S) {
  if (N < 1 || rows < 1 || S < 1) return V3A_ERR_SHAPE;
  return (long)N * rows * S * 3;
}

extern "C" int v3a_clip_preprocess(const v3a_clip_preprocess_args* a, void* stream) {
  if (!a) return V3A_ERR_ARG;
  if (!a->src || !a->x_bounds || !a->x_coeffs || !a->y_bounds || !a->y_coeffs || !a->lut || !a->patches_hi || !a->patches_lo) return V3A_ERR_ARG;
  if (a->N < 1 || a->H < 1 || a->W < 1 || a->S < 1 || a->P < 1 || a->S % a->P || a->kx < 1 || a->ky < 1) return V3A_ERR_SHAPE;
  if (a->ldk < 3 * a->P * a->P || a->ldk % 8) return V3A_ERR_SHAPE;
  if (a->row0 < 0 || a->rows < 1 || a->row0 + a->rows > a->H) return V3A_ERR_SHAPE;
  const long need = v3a_clip_preprocess_workspace_bytes(a->N, a->rows, a->S);
  if (!a->workspace || a->workspace_bytes < need) return V3A_ERR_WORKSPACE;
  ResizeP p{(const unsigned char*)a->src, (unsigned char*)a->workspace, a->x_bounds, a->x_coeffs, a->y_bounds, a->y_coeffs, a->lut,
            (char*)a->patches_hi, (char*)a->patches_lo, (unsigned char*)a->out_u8, a->out_f32,
            a->N, a->H, a->W, a->S, a->P, a->ldk, a->kx, a->ky, a->row0, a->rows};
  const long t1 = (long)a->N * a->rows * a->S, t2 = (long)a->N * a->S * a->S;
  const long b1 = (t1 + THREADS - 1) / THREADS, b2 = (t2 + THREADS - 1) / THREADS;
  if (b1 > 0x7fffffffL || b2 > 0x7fffffffL) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(clip_resize_h_kernel, dim3((unsigned)b1), dim3(THREADS), 0, (hipStream_t)stream, p);
  if (hipGetLastError() != hipSuccess) return V3A_ERR_LAUNCH;
  hipLaunchKernelGGL(clip_resize_v_kernel, dim3((unsigned)b2), dim3(THREADS), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_clip_rows(const float* src, int src_rows, const int* ids, const float* cls, const float* pos, float* out, long M, int S,
                             int d, void* stream) {
  if (!src || !out) return V3A_ERR_ARG;
  if (ids && cls) return V3A_ERR_ARG;
  if (M < 1 || S < 1 || d < 4 || d % 4 || src_rows < 1) return V3A_ERR_SHAPE;
  if (cls && (S < 2 || M % S || (M / S) * (S - 1) > src_rows)) return V3A_ERR_SHAPE;
  if (!ids && !cls && M > src_rows) return V3A_ERR_SHAPE;
  RowsP p{src, ids, cls, pos, out, M, S, d, src_rows};
  const long blocks = (M * (d / 4) + THREADS - 1) / THREADS;
  if (blocks > 0x7fffffffL) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(clip_rows_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_attention_f32(const float* q, const float* k, const float* v, int ld, void* o_hi, void* o_lo, float* o_f32, int ldo,
                                 const int* lens, int B, int S, int H, int hd, float scale, int causal, void* stream) {
  if (!q || !k || !v || (!o_f32 && !o_hi) || (!o_hi != !o_lo)) return V3A_ERR_ARG;
  if (hd != HD || B < 1 || B > 65535 || H < 1 || H > 65535 || S < 1 || S > 1024) return V3A_ERR_SHAPE;
  if (ld < H * HD || ld % 4 || ldo < H * HD || ldo % 8) return V3A_ERR_SHAPE;
  AttnP p{q, k, v, (char*)o_hi, (char*)o_lo, o_f32, lens, ld, ldo, B, S, H, causal ? 1 : 0, scale};
  hipLaunchKernelGGL(attention_f32_kernel, dim3((S + QT - 1) / QT, H, B), dim3(QT), 0, (hipStream_t)stream, p);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}

extern "C" int v3a_clip_score(const float* image_emb, const float* text_emb, int F, int D, double* scores, double* mean, void* stream) {
  if (!image_emb || !text_emb || !scores) return V3A_ERR_ARG;
  if (F < 1 || D < 1) return V3A_ERR_SHAPE;
  hipLaunchKernelGGL(clip_score_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, image_emb, text_emb, F, D, scores, mean);
  return hipGetLastError() == hipSuccess ? V3A_OK : V3A_ERR_LAUNCH;
}
