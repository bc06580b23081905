/*
 * libvist3a_hip.so — C ABI of the MI355X (gfx950) kernels behind the VIST3A text->3DGS inference path.
 *
 * The reference (gohyojun15/VIST3A) has no FFI layer: its "operator API" for this path is the PyTorch
 * nn.Module surface.  Every entry point below replaces the ATen/cuDNN/SDPA call(s) the
 * reference reaches at the cited file:line; the Python host in vist3a_amd/ calls them through ctypes with
 * raw device pointers.  Conventions:
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless noted;
 *   - `stream` is a hipStream_t passed as void*; calls are stream-ordered, re-entrant, allocate nothing;
 *   - return 0 on success, negative V3A_ERR_* otherwise; never throws;
 *   - bf16 tensors are raw uint16 storage (round-to-nearest-even, same as torch.bfloat16).
 *
 * MEMORY CONTRACT.  An entry point reads and writes only the [rows, cols] region of each operand and the first
 * `workspace_bytes` bytes of its workspace.  Row strides (ld*), batch / segment strides and row scatters (out_row_*) say where
 * the rows lie, never how much of one may be touched: columns cols .. ld, rows the scatter skips, the gap between two batch
 * items or two slabs, and everything before the first and after the last element belong to the caller - typically to the
 * neighbouring operand of a fused buffer - and are neither loaded (their contents, NaN included, cannot reach a result) nor
 * stored.  In-place operands (residual aliasing C, y aliasing x, v3a_qknorm_rope2d, v3a_adam_step's p / m / v) follow the same
 * rule for their padding.  Where an entry point by design owns MORE than the region, its comment states the exact extent:
 *   - v3a_attn_args.vt / v3a_attn_fp8_args.vt: every V^T row is READ up to the next multiple of 64 keys past each batch item's
 *     Nk; the values there must be finite and do not reach the result; nothing beyond is read (with kv_seg a segment is a
 *     whole number of 64-key tiles - kv_seg % 64 == 0, Nk % kv_seg == 0 - so exactly the segment is read);
 *   - v3a_xattn_probs_args.p: the region is [B * Nq, H * Lkp]; columns Nk <= j < Lkp of every head are WRITTEN (zeros);
 *   - packed convolution weights (w [Cout][Kpad], ktab [Kpad / 8], w_halo): read in full, padding chunks included.
 * tests/test_guard_bands_gpu.py holds the entry points to this: every tensor carved out of an all-0xFF arena with guard bands,
 * results bit-equal to those on tight tensors, guard bytes and inputs unchanged.
 */
#ifndef VIST3A_HIP_H
#define VIST3A_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define V3A_OK 0
#define V3A_ERR_ARG (-1)
#define V3A_ERR_SHAPE (-2)
#define V3A_ERR_LAUNCH (-3)
#define V3A_ERR_WORKSPACE (-4)

int v3a_abi_version(void);            /* bumps whenever a signature changes (currently 37) */
const char* v3a_build_info(void);     /* "gfx950 <date> <compiler>" */

/* ------------------------------------------------------------------------------------------------
 * GEMM  C[M,N] = epilogue( A[M,K] . B[N,K]^T )      bf16 inputs, fp32 MFMA accumulation
 * replaces torch.nn.Linear / F.linear under bf16 autocast:
 *   DiT   : diffusers==0.33.1 WanAttnProcessor2_0 to_q/to_k/to_v/to_out, FeedForward net.0.proj/net.2,
 *           condition_embedder, proj_out (call site /root/reference/inference_t23d.py:94-103)
 *   recon : vggt/layers/attention.py:51,77 (qkv, proj), vggt/layers/mlp.py:33-38 (fc1, fc2)
 * Epilogue order (each stage optional):  v = acc + bias ; v = bf16(v) ; v = act(v) ; v = bf16(v) ;
 *   v = v * scale ; [v = bf16(v)] ; v = v + residual ; store as bf16 or f32.
 * These rounding points are the ones CUDA autocast produces in the reference.
 * ---------------------------------------------------------------------------------------------- */
enum {
  V3A_ACT_NONE = 0,
  V3A_ACT_GELU_TANH = 1, /* FeedForward(activation_fn="gelu-approximate") */
  V3A_ACT_GELU_ERF = 2,  /* vggt/layers/mlp.py nn.GELU */
  V3A_ACT_SILU = 3,
  V3A_ACT_RELU = 4,
  V3A_ACT_QUICK_GELU = 5 /* x * sigmoid(1.702 x): CLIP's MLP; the fp32 epilogue of v3a_conv_split only */
};
enum {
  V3A_GEMM_BIAS_ROW = 1 << 0,     /* bias indexed by output row (used for the V^T = Wv.X^T form) */
  V3A_GEMM_SCALE_PER_BATCH = 1 << 1, /* scale[(row / rows_per_batch) * scale_stride + col] (AdaLN gate) else scale[col] (LayerScale) */
  V3A_GEMM_ROUND_AFTER_SCALE = 1 << 2, /* round v*scale to bf16 before adding the residual */
  V3A_GEMM_RES_F32 = 1 << 3,      /* residual is float32 (aggregator residual stream) else bf16 */
  V3A_GEMM_OUT_F32 = 1 << 4,      /* store float32 else bf16 */
  V3A_GEMM_NO_ROUND_ACC = 1 << 5, /* reserved (not implemented: accumulators are parked as bf16) */
  V3A_GEMM_RELU_OUT = 1 << 6      /* ReLU after the residual adds (DPT ResidualConvUnit chains) */
};
typedef struct {
  const void* A;        /* bf16 [M, lda] */
  const void* B;        /* bf16 [N, ldb] (nn.Linear weight layout) */
  void* C;              /* bf16 or f32 [M, ldc] */
  const float* bias;    /* f32 [N] (or [M] with BIAS_ROW); may be NULL */
  const void* residual; /* bf16/f32 [M, ldr]; may be NULL; may alias C */
  const float* scale;   /* f32; may be NULL */
  int M, N, K;          /* K % 64 == 0, lda/ldb % 8 == 0, ldc % 8 == 0 */
  int lda, ldb, ldc, ldr;
  int rows_per_batch, scale_stride;
  int act;              /* V3A_ACT_* */
  int flags;            /* V3A_GEMM_* */
  int tile;             /* -1 = auto, else index into the tile table (bench/tuning; all tiles give bit-identical results): 0-5 lockstep, 6-8 ping-pong,
                         * 9-11 small, 12 128x96, 13 transposed tail, 14 one wave per SIMD (hand-scheduled K loop), 15-21 deep-ring forms of the
                         * small / medium tiles (shard-size launches); v3a_gemm_tile_name(i) names them */
  const void* residual2; /* optional second residual, bf16 [M, ldr2] */
  int ldr2;
  int res_row_mod;      /* > 0: `residual` row index is (row % res_row_mod): broadcast table (positional embedding) */
  int out_row_group, out_row_skip, out_row_off; /* group > 0: output row = row + (row / group) * skip + off */
  int split_k;          /* > 1 (v3a_gemm_bf16_nt only): K is cut into split_k equal slices (K % (64 * split_k) == 0) computed side by side
                         * into bf16 partials, summed in slice order by a second launch that applies the epilogue - for problems with
                         * few output tiles and a long K (a sequence-parallel shard's FFN2).  Deterministic; not bit-identical to 0 / 1. */
  void* workspace;      /* split_k > 1: v3a_gemm_split_workspace_bytes(M, N, split_k) bytes */
  int batch;            /* > 1 (v3a_gemm_bf16_nt, not with split_k): `batch` equally shaped problems side by side in ONE launch; problem z
                         * reads A + z * a_batch_stride, B + z * b_batch_stride, writes C + z * c_batch_stride, adds residual +
                         * z * res_batch_stride (strides in ELEMENTS of the respective tensor; 0 = shared).  bias / scale / residual2 are
                         * shared.  Used for per-head and per-prompt operands (the cached-context cross-attention of the DiT: one B
                         * operand per CFG batch item) where separate launches would each fill a fraction of the chip. */
  long a_batch_stride, b_batch_stride, c_batch_stride, res_batch_stride;
  float* row_sumsq;     /* optional by-product (v3a_gemm_bf16_nt; N % 32 == 0, act NONE, no scale, no BIAS_ROW, no split_k): f32 [M][N / 32],
                         * entry [m][n / 32] = sum over the 32-column block of bf16(acc + bias)^2 - the statistics of an RMS norm that the
                         * CONSUMER applies (v3a_xattn_probs_args.q_row_sumsq), so the normalisation pass over the output disappears.
                         * Independent of the tile shape (bit-identical for every tile); with `batch` the rows of problem z are
                         * offset by z * M. */
  void* C_t;            /* optional TRANSPOSED TAIL (v3a_gemm_bf16_nt): output columns n >= t_col0 are written to C_t[(n - t_col0) * ldct + m] (bf16)
                         * instead of C; columns below t_col0 go to C as usual (ldc may be t_col0).  For the fused q | k | v projection of a DiT
                         * block (diffusers WanAttnProcessor2_0 to_q / to_k / to_v, call site /root/reference/inference_t23d.py:94-103): B =
                         * (Wq | Wk | Wv) stacked, q | k land row-major in C and V^T - what the flash kernel reads - in C_t, as 768 tiles = three
                         * full rounds of ONE launch.  t_col0 % 192 == 0, ldct % 8 == 0, M % 8 == 0; bias only (no act / scale / residual / row
                         * scatter / split_k / batch / row_sumsq).  Bit-identical to the two separate GEMMs. */
  int ldct, t_col0;
} v3a_gemm_args;
int v3a_gemm_bf16_nt(const v3a_gemm_args* args, void* stream);
size_t v3a_gemm_split_workspace_bytes(int M, int N, int split_k);
int v3a_gemm_num_tiles(void);
int v3a_gemm_pick_tile(int M, int N);   /* the tile index tile=-1 resolves to (profiling / roofline bookkeeping) */
int v3a_gemm_pick_tile_act(int M, int N, int act);   /* ... for a launch with activation `act` (ties between mirrored tiles depend on it) */
/* ... the tile a launch REALLY runs on: `mult` = batch / split_k problems side by side, `has_tail` != 0 when C_t is set (the
 * transposed-tail tile whatever M, N).  An explicit `tile` >= 0 that contradicts C_t is rejected with V3A_ERR_ARG by the launch. */
int v3a_gemm_pick_tile_ex(int M, int N, int act, int mult, int has_tail);
const char* v3a_gemm_tile_name(int tile);

/* e4m3 (OCP fp8) form of v3a_gemm_bf16_nt for BASELINE config #4 (Wan-14B: "MFMA bf16/fp8 GEMMs for the attention/FFN contractions"):
 *   C[m][n] = epilogue( a_scale[m] * b_scale[n] * sum_k A8[m][k] * B8[n][k] )        (fp32 accumulation, scales multiplied first)
 * A8 [M][lda], B8 [N][ldb] are e4m3 BYTES (K % 128 == 0, lda/ldb % 16 == 0) as written by v3a_quantize_fp8_rows (per-row dynamic
 * scales: activations per token, weights per output channel).  Everything after the dequantisation - bias, activation, gate scale,
 * residuals, output type, row scatter, flags - is the bf16 GEMM's epilogue, field for field (g.*).  The main loop is the ping-pong
 * loop of v3a_gemm_bf16_nt with v_mfma_scale_f32_32x32x64_f8f6f4 (unit block scales) in place of the bf16 MFMA: same bytes per
 * LDS row, twice the K per phase.  g.tile: -1 = heuristic, or 0 .. v3a_gemm_fp8_num_tiles()-1.
 * v3a_quantize_fp8_rows: scale[r] = max(amax_r, 1e-12) / 448 (IEEE), y[r][c] = e4m3(clamp(x[r][c] * (1 / scale[r]), +-448)), RNE.
 * x bf16 [rows][ldx] (cols % 8 == 0), y bytes [rows][ldy], scale fp32 [rows]. */
typedef struct {
  v3a_gemm_args g;          /* A, B: e4m3 bytes; lda, ldb, K in elements (= bytes) */
  const float* a_scale;     /* [M] */
  const float* b_scale;     /* [N] */
} v3a_gemm_fp8_args;
int v3a_gemm_fp8_nt(const v3a_gemm_fp8_args* args, void* stream);
int v3a_gemm_fp8_num_tiles(void);
int v3a_gemm_fp8_pick_tile(int M, int N);
const char* v3a_gemm_fp8_tile_name(int tile);
int v3a_quantize_fp8_rows(const void* x, void* y, float* scale, long rows, int cols, int ldx, int ldy, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Convolution (1-D/2-D/3-D, stride, zero or replicate padding, causal-in-time, optional fused nearest-exact 2x
 * spatial upsample of the input) as an implicit GEMM on the same MFMA main loop and epilogue as v3a_gemm_bf16_nt.
 * replaces nn.Conv3d / nn.Conv2d at
 *   /root/reference/utils/wan_utils.py:96-147 (WanCausalConv3d), :202-330 (WanResample upsample + Conv2d, time_conv)
 *   /root/reference/models/stitching_layer_builder.py:32-42 (stitching Conv3d, padding_mode="replicate")
 *   /root/reference/third_party_model/anysplat/src/model/encoder/vggt/heads/dpt_head.py (DPT convs)
 * Activations are CHANNELS-LAST: x[T][H][W][Cin] bf16, y[oT*oH*oW][ldy] (first Cout columns written).
 * Weights are pre-packed  w[Cout][Kpad],  k = ((dt*kH + dh)*kW + dw)*Cin + c, zero padded to Kpad % 64 == 0.
 * ktab[Kpad/8] describes each 8-channel K chunk:  c | dw<<16 | dh<<20 | dt<<24 | 1<<31 (0 for padding chunks).
 * Tap (dt,dh,dw) of output (t,h,w) reads input (t*sT+dt-pT, h*sH+dh-pH, w*sW+dw-pW); out-of-range taps read zero
 * (or the clamped coordinate when `replicate`).  With ups2 the (H,W) coordinates address the 2x upsampled image.
 * Epilogue = the GEMM epilogue (bias per Cout, act, scale per Cout, residual [M][ldr], bf16/f32 out).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* x; const void* w; const int* ktab; void* y;
  const float* bias; const void* residual; const float* scale;
  int T, H, W, Cin;
  int oT, oH, oW, Cout, Kpad;
  int sT, sH, sW;
  int pT, pH, pW;
  int ups2, replicate;
  int ldy, ldr;
  int act, flags, tile;
  const void* residual2; int ldr2; int res_row_mod;
  int out_row_group, out_row_skip, out_row_off;   /* as in v3a_gemm_args */
  /* Optional second packing of the same weights for the HALO-TILE kernel (csrc/conv_halo.hip): 3x3 spatial taps, kT = halo_kT in
   * {1, 3} (causal in time: pT = kT - 1), stride 1, zero padding 1, Cin % 48 == 0, Cout % 96 == 0, oH % 16 == 0, oW % 32 == 0.
   * The input patch of a 16 x 32-pixel output tile is staged once in LDS and the nine spatial taps are read as shifted views of it
   * (the Wan VAE decoder's wide-image layers, /root/reference/utils/wan_utils.py:96-147, 202-330, 333-425).
   * Layout: w_halo[Cout/96][kT][Cin/48][9 = dh*3+dw][96 rows n][48 k] bf16, where the six 16-byte chunks of a row are stored
   * rotated: logical chunk c of row n sits at position (c + 3*((n >> 3) & 1)) % 6 (the kernel's LDS bank layout; the slab is
   * copied to LDS verbatim).  NULL = implicit-GEMM path only.  v3a_conv_bf16 takes the halo kernel when w_halo is set, the layer
   * has this form, tile < 0 and v3a_conv_halo_tiles(args) >= 512; tile == -2 forces it, tile == -3 forbids it.
   * H-STRIPS (a spatially sharded image: wan/vae.py decode_cl_sharded): the stored input may carry ONE explicit halo row above and below
   * every frame and be convolved VALID in H - pH = 0 with H = oH + 2, or with ups2 pH = -1 with 2 (H - 2) = oH (output row j reads rows
   * j + 1 + dh of the 2x upsampled haloed strip).  Both kernels take it (negative pH is plain arithmetic in the implicit GEMM). */
  const void* w_halo; int halo_kT;
} v3a_conv_args;
int v3a_conv_bf16(const v3a_conv_args* args, void* stream);
long v3a_conv_halo_tiles(const v3a_conv_args* args);   /* workgroups the halo kernel would launch; 0 = layer not of its form */

/* ------------------------------------------------------------------------------------------------
 * fp32-EQUIVALENT convolution on the bf16 matrix pipe ("split bf16"), for the layers the reference runs with autocast OFF:
 *   /root/reference/models/anysplat_stitched.py:335 (`with torch.amp.autocast("cuda", enabled=False)` around camera / depth / Gaussian heads)
 *   /root/reference/third_party_model/anysplat/src/model/encoder/vggt/heads/dpt_head.py:185-309 (DPT trunk + output convs, fp32 weights:
 *   utils/utils_for_thirdparty.py:53-69), .../encoder/heads/vggt_dpt_gs_head.py:122-176.
 * An fp32 tensor t travels as an unevaluated PAIR of bf16 planes of its shape, t = hi + lo with hi = bf16(t), lo = bf16(t - hi)
 * (|t - hi - lo| <= 2^-17 |t|).  With x = xh + xl and w = wh + wl the convolution is the sum of three bf16 products with fp32
 * accumulation,  xl.wh + xh.wl + xh.wh  (the dropped xl.wl term is <= 2^-16 relative), laid out ALONG K of one implicit GEMM:
 *   w[Cout][Kpad]: three consecutive copies of the tap-major K range of v3a_conv_args, holding (wh | wl | wh);
 *   ktab: the chunk table of the three ranges, bit 28 set where the chunk reads the LO plane of x (first range), clear for the hi plane.
 * Everything that follows the accumulation stays in fp32: v = act(acc + bias) (act NONE, RELU or QUICK_GELU) + residual + residual2 ; [RELU_OUT] ;
 * stored as f32 (V3A_GEMM_OUT_F32) or split into the (y, y_lo) planes.  residual: f32 [.., ldr] with V3A_GEMM_RES_F32 (a table, see
 * res_row_mod) else a pair (c.residual, residual_lo); residual2: a pair.  c.scale must be NULL.  Geometry fields (T..pW, ups2, replicate,
 * ldy, out_row_*) as in v3a_conv_args; both planes of a pair share strides.
 * HALO-TILE form (csrc/conv_halo_split.hip) for 3x3 layers with stride 1, zero padding 1, kT = 1, Cin % 16 == 0, Cout % 32 == 0,
 * oH % 16 == 0, oW % 32 == 0: the (hi, lo) input patch of a 16 x 32-pixel output tile is staged once in LDS, the nine taps are shifted
 * views of it and every fragment feeds all three products.  c.w_halo = the second packing
 *   [Cout/BN][Cin/16][9 = dh*3+dw][2 = hi, lo][BN rows n][16 k] bf16,  BN = v3a_conv_split_halo_bn(Cout)  (128, 64 or 32),
 * where the two 16-byte chunks of a row are swapped when (n >> 3) & 1 (the kernel's LDS bank layout; slabs are copied verbatim), and
 * c.halo_kT = 1.  Taken when w_halo is set, the layer has this form, tile < 0 and v3a_conv_split_halo_tiles(args) >= 128; tile == -2
 * forces it, tile == -3 forbids it, tile >= 0 selects that implicit-GEMM tile.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  v3a_conv_args c;            /* x, y, residual, residual2 = the HI planes */
  const void* x_lo; void* y_lo; const void* residual_lo; const void* residual2_lo;
} v3a_conv_split_args;
int v3a_conv_split(const v3a_conv_split_args* args, void* stream);
int v3a_conv_split_halo_bn(int Cout);                               /* output channels per workgroup of the halo packing; 0 = none */
long v3a_conv_split_halo_tiles(const v3a_conv_split_args* args);    /* workgroups the halo form would launch; 0 = layer not of its form */
/* Row / pixel passes between the split convolutions (csrc/pair.hip), fp32 arithmetic, pair in / pair out:
 *   v3a_split_f32        x f32 [n] (n % 8 == 0) -> (hi, lo)
 *   v3a_layernorm_pair   F.layer_norm of f32 rows x[row(m)][0..d) (row(m) = m + (m / in_row_group) * in_row_skip + in_row_off when
 *                        in_row_group > 0), affine weight / bias f32 [d] or NULL -> pair rows [M][ldy]; d % 8 == 0, d <= 2048
 *                        (dpt_head.py:213-216 `self.norm` on the tapped tokens)
 *   v3a_bilinear_cl_pair v3a_bilinear_cl on pairs: x [T][h][w][C] -> y [T][H][W][C], + optional pair `add` [T][H][W][C], + optional f32
 *                        `table` [H*W][C] broadcast over T (dpt_head.py:291-309,460-466, vggt_dpt_gs_head.py:166) */
int v3a_split_f32(const float* x, void* hi, void* lo, long n, void* stream);
int v3a_layernorm_pair(const float* x, void* y_hi, void* y_lo, const float* weight, const float* bias, int M, int d, int ldx, int ldy,
                       float eps, int in_row_group, int in_row_skip, int in_row_off, void* stream);
int v3a_bilinear_cl_pair(const void* x_hi, const void* x_lo, void* y_hi, void* y_lo, const void* add_hi, const void* add_lo,
                         const float* table, int T, int h, int w, int H, int W, int C, int align_corners, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Flash attention forward (non-causal, no mask, no dropout), bf16 in/out, fp32 softmax.
 * replaces F.scaled_dot_product_attention at
 *   diffusers==0.33.1 WanAttnProcessor2_0 (DiT self/cross attention; call site inference_t23d.py:94-103)
 *   /root/reference/third_party_model/anysplat/src/model/encoder/vggt/layers/attention.py:64-69
 * Q,K: [B][N][H*D] with row stride ld* ; V is passed TRANSPOSED: vt[(h*D+d)*ldvt + b*vt_batch_stride + key],
 * readable and finite up to the next multiple of 64 keys past each batch's Nk.  D in {64,128}.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* q; const void* k; const void* vt; void* o;   /* bf16 */
  long q_batch_stride, k_batch_stride, vt_batch_stride, o_batch_stride; /* elements */
  int ldq, ldk, ldvt, ldo;                                  /* elements */
  int B, H, Nq, Nk, D;
  float scale;                                              /* softmax scale, normally D^-0.5 */
  int kv_period, kv_valid;  /* kv_period > 0: key k participates only if (k % kv_period) < kv_valid (per-frame row padding);
                               not together with rel_bias / key_bias (V3A_ERR_ARG) */
  const float* rel_bias;    /* optional (D = 64 only): additive bias by relative position, fp32 [H][rel_bias_stride], entry
                             * (key - query + rel_bias_center) is added to scale*q.k — T5/UMT5 relative attention bias */
  int rel_bias_stride, rel_bias_center;
  const float* key_bias;    /* optional (D = 128 only): additive per-key bias, fp32 [B][key_bias_stride >= Nk], added to scale*q.k.
                             * Used to merge the identical zero-padding keys of a prompt into one key carrying log(count). */
  int key_bias_stride;
  int key_bias_first;       /* keys < key_bias_first have zero bias (their tiles skip the bias loads); 0 = any key may carry bias */
  int kv_seg;               /* optional (D = 128 only): keys of a batch item are split into segments of kv_seg keys (multiple of 64, divides Nk),
                             * segment s of K at k + s * k_seg_stride, of V^T at vt + s * vt_seg_stride (elements): the all-gathered per-rank
                             * slabs of sequence-parallel attention are read in place.  Inside a segment: ldk / k_batch_stride / ldvt /
                             * vt_batch_stride as usual */
  long k_seg_stride, vt_seg_stride;
  int kv_split;             /* optional (D = 128 only): > 1 divides the key tiles of every query block among kv_split workgroups and
                             * merges their partial softmaxes in a second launch (fixed order: deterministic, but not bit-identical to
                             * kv_split <= 1).  For launches too small to occupy the chip: a sequence-parallel shard has N / P query rows
                             * but walks all N keys per workgroup. */
  void* workspace;          /* kv_split > 1: v3a_attention_split_workspace_bytes(B, H, Nq, D, kv_split) bytes */
} v3a_attn_args;
int v3a_attention_fwd_bf16(const v3a_attn_args* args, void* stream);
size_t v3a_attention_split_workspace_bytes(int B, int H, int Nq, int D, int kv_split);

/* ------------------------------------------------------------------------------------------------
 * Cross-attention PROBABILITIES over a short per-prompt key set (csrc/xattn_probs.hip): the first half of the cached-context form
 *     attn2(x) = softmax(q K^T) V Wo^T + bo = sum_h P_h (V_h Wo_h^T) + bo
 * of diffusers==0.33.1 WanTransformerBlock.attn2 (call site /root/reference/inference_t23d.py:94-103).  K, V depend on the prompt only:
 * the host caches (V_h Wo_h^T) per prompt and v3a_gemm_bf16_nt (batch = CFG items, K = H * Lkp) finishes the layer.
 *   p[b][m][h * Lkp + j] = bf16( softmax_j( scale * q[b][m][h*D:(h+1)*D] . k[b][j][h*D:(h+1)*D] + key_bias[b][j] ) ),  j < Nk;  0 for
 *   Nk <= j < Lkp.  D = 128, Nk <= 128, Lkp % 16 == 0, Nk <= Lkp <= 128, ldp >= H * Lkp.  key_bias (optional, f32 [B][key_bias_stride])
 *   is added for keys >= key_bias_first (the merged zero-padding key carries log(count), v3a_attn_args.key_bias).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* q; const void* k; void* p;      /* bf16 */
  const float* key_bias;
  long q_batch_stride, k_batch_stride, p_batch_stride;   /* elements */
  int ldq, ldk, ldp;
  int B, H, Nq, Nk, D, Lkp;
  int key_bias_stride, key_bias_first;
  float scale;
  const float* q_row_sumsq;   /* optional: q is NOT yet RMS-normalised; f32 [B * Nq rows of q][q_sumsq_parts] partial sums of squares of each
                               * full q row (v3a_gemm_args.row_sumsq of the projection that produced q: parts = H * D / 32).  The kernel
                               * multiplies the scores of query m by rsqrt(sum(parts) / (H * D) + q_eps) - the per-row factor of
                               * diffusers' RMSNorm "across heads"; its per-column weight must be folded into k by the caller. */
  int q_sumsq_parts;
  float q_eps;
} v3a_xattn_probs_args;
int v3a_xattn_probs_bf16(const v3a_xattn_probs_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp8 (OCP e4m3) flash attention forward on the block-scaled MFMA (K = 64, twice the bf16 rate): the self-attention launch of
 * BASELINE config #4 (Wan-14B; model choice at /root/reference/utils/argument.py:399, /root/reference/inference_t23d.py:73).
 * The reference computes this attention in bf16 (F.scaled_dot_product_attention under autocast): this entry is an opt-in
 * precision mode whose rounding points are pinned by the oracle's e4m3 emulation (oracle/wan_dit.py attention_fp8_emulated).
 * q, k: e4m3 bytes [B][N][H*128] (row stride ld* BYTES); vt: e4m3 bytes [H*128][B*vt_batch_stride + key], readable up to the next
 * multiple of 64 keys; o: bf16.  Stored values are x / *_scale; D must be 128.
 * v3a_quantize_fp8: y[r][c] = e4m3(x[r][c] / scale), RNE, clamped to +-448; x bf16 [rows][ldx], y bytes [rows][ldy], cols % 16 == 0.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* q; const void* k; const void* vt; void* o;
  long q_batch_stride, k_batch_stride, vt_batch_stride, o_batch_stride;   /* elements of the respective tensor */
  int ldq, ldk, ldvt, ldo;
  int B, H, Nq, Nk, D;
  float scale;                      /* softmax scale, normally D^-0.5 */
  float q_scale, k_scale, v_scale;  /* per-tensor quantisation scales */
  int kv_seg;               /* as in v3a_attn_args: K / V^T read in place from per-rank slabs; k_seg_stride / vt_seg_stride in BYTES */
  long k_seg_stride, vt_seg_stride;
  int kv_split;             /* as in v3a_attn_args (workspace: v3a_attention_split_workspace_bytes(B, H, Nq, 128, kv_split)) */
  void* workspace;
} v3a_attn_fp8_args;
int v3a_attention_fwd_fp8(const v3a_attn_fp8_args* args, void* stream);
int v3a_quantize_fp8(const void* x, void* y, long rows, int cols, int ldx, int ldy, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm in fp32 (+ optional affine) (+ optional AdaLN modulation  y = LN(x)*(1+scale[b])+shift[b]).
 * replaces diffusers==0.33.1 FP32LayerNorm in WanTransformerBlock (norm1/norm2/norm3) and norm_out,
 * and nn.LayerNorm at /root/reference/third_party_model/anysplat/src/model/encoder/vggt/layers/block.py:41,47.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const void* x; void* y;             /* [M, ld*]; bf16 unless *_is_f32 */
  const float* weight; const float* bias;   /* [d] or NULL */
  const float* scale; const float* shift;   /* [nbatch, mod_stride] or NULL (both or neither) */
  int M, d, ldx, ldy;
  int rows_per_batch, mod_stride;
  float eps;
  int x_is_f32, y_is_f32;
  int in_row_group, in_row_skip, in_row_off;    /* group > 0: logical row m reads x row m + (m/group)*skip + off */
  int out_row_group, out_row_skip, out_row_off; /* same for the output (gather/scatter of per-frame token blocks) */
  int rms;                                      /* 1: RMS norm, no mean subtraction (T5LayerNorm of the UMT5 text encoder) */
  float* y_fp8_scale;                           /* non-NULL: y is e4m3 BYTES [rows][ldy] = v3a_quantize_fp8_rows of the bf16 result, its
                                                   per-row scales written here (fp8 GEMM mode: saves the separate quantisation pass) */
} v3a_layernorm_args;
int v3a_layernorm(const v3a_layernorm_args* args, void* stream);

/* RMSNorm across the full width + optional RoPE (complex multiply of adjacent pairs, per head).
 * replaces diffusers==0.33.1 RMSNorm (attn.norm_q / norm_k, "rms_norm_across_heads") followed by
 * WanAttnProcessor2_0.apply_rotary_emb.  rope = float [tokens_per_batch][head_dim/2][2] = (cos, sin). */
typedef struct {
  const void* x; void* y;     /* bf16 [M, ld*]; y may alias x */
  const float* weight;        /* [d] */
  const float* rope;          /* or NULL */
  int M, d, ldx, ldy, head_dim, tokens_per_batch;
  float eps;
  const float* weight2;       /* non-NULL: a SECOND column block x[:, d:2d] -> y[:, d:2d] normalised with weight2 in the same launch
                               * (q and k of the fused q|k projection: one launch instead of two) */
  float y_fp8_scale;          /* > 0: y is e4m3 BYTES [M, ldy] (ldy in bytes) holding e4m3(bf16(result) / y_fp8_scale), the operand format of
                               * v3a_attention_fwd_fp8 (= this call followed by v3a_quantize_fp8, bit for bit, in one pass); y != x */
} v3a_rmsnorm_rope_args;
int v3a_rmsnorm_rope(const v3a_rmsnorm_rope_args* args, void* stream);

/* Channel norm over channels-last pixels (+ optional SiLU): mode 0 RMSNorm(eps); mode 1 = F.normalize(x,dim=C)
 * * sqrt(C) * gamma (+ bias), i.e. WanRMS_norm (/root/reference/utils/wan_utils.py:150-184) fused with the SiLU that
 * follows it in WanResidualBlock (:370-372,:399-400) and WanDecoder3d (:873-874). bf16 in / bf16 out. */
typedef struct {
  const void* x; void* y;
  const float* weight; const float* bias;   /* [d]; bias may be NULL */
  long M; int d, ldx, ldy;
  float eps; int mode; int act;             /* act: V3A_ACT_NONE or V3A_ACT_SILU */
} v3a_rownorm_args;
int v3a_rownorm_act(const v3a_rownorm_args* args, void* stream);

/* P[M,N] (bf16) = softmax(scale * S[M,N]) (f32), row-wise.  The VAE mid-block's single 384-wide head
 * (/root/reference/utils/wan_utils.py:428-475) runs as GEMM -> this -> GEMM. */
int v3a_softmax_rows(const float* s, void* p, int M, int N, int lds, int ldp, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stitched-reconstruction glue.  Channels-last (CL) tensors are [T][H][W][C].
 * ---------------------------------------------------------------------------------------------- */
/* per-head LayerNorm(64, affine) on q and k + 2-D RoPE, in place on the fused [q|k] buffer qk[M][ld] (q cols 0..C-1,
 * k cols C..2C-1).  vggt/layers/attention.py:56-61, rope.py:154-188.  cos_sin = f32 [maxpos][16][2]; token row r has
 * p = r % rows_per_frame; p < n_special or p >= n_valid -> position 0, else patch p-n_special -> (y,x)+1 on a wp-wide grid. */
int v3a_qknorm_rope2d(void* qk, int M, int ld, int C, const float* q_w, const float* q_b, const float* k_w, const float* k_b,
                      const float* cos_sin, int rows_per_frame, int n_special, int n_valid, int wp, float eps, void* stream);
/* latent z[C][Tl][H][W] f32 -> CL bf16 [4(Tl-1)+1][H][W][C], align_corners=True lerp in T (models/stitched_model.py:92-107) */
int v3a_latent_upsample_t_cl(const float* z, void* y, int C, int Tl, int H, int W, void* stream);
/* bilinear resize of a CL bf16 stack (+ bf16 addend [T*H*W][C]) (+ f32 table [H*W][C] broadcast over T) (+ ReLU)
 * vggt/heads/dpt_head.py:460-466 (align_corners=True), inference_t23d.py:118-123 (False) */
int v3a_bilinear_cl(const void* x, void* y, const void* add, const float* table, int T, int h, int w, int H, int W, int C,
                    int align_corners, int relu, int out_f32, void* stream);
/* depth head activation + unprojection: raw[M][ld] f32 (col0 log-depth, col1 log-conf) -> depth[M]=exp, conf[M]=1+exp,
 * pts[M][3] world points.  cam[S][16] = {fx,fy,cx,cy, R^T (9, row-major), -R^T t (3)}.  head_act.py:61-112, geometry.py:10-58 */
int v3a_depth_unproject(const float* raw, int ld, const float* cam, float* depth, float* conf, float* pts, int S, int H, int W,
                        void* stream);
/* voxel fusion: see csrc/voxel.hip.  feat[M][ldf] f32 holds nfeat feature columns (0..nfeat-1) and the raw confidence at
 * conf_col.  Outputs sized for the worst case U = M: keys_out[M][3] i32 (lexicographically sorted unique voxel coords),
 * inverse_out[M] i32, counts_out[M] i32, voxel_pts[M][3], voxel_feat[M][ldo]; *num_voxels = U (device int).
 * *status (device int) != 0 if a coordinate fell outside [-2^20, 2^20) voxels.  anysplat.py:298-335
 * The call SYNCHRONISES `stream` once (the per-axis coordinate range is read back to size the sort key): not capturable in a hipGraph. */
long v3a_voxelize_workspace_bytes(long M);
int v3a_voxelize_fuse(const float* pts, const float* feat, int ldf, int nfeat, int conf_col, long M, float voxel_size,
                      void* workspace, long workspace_bytes, int* keys_out, int* inverse_out, int* counts_out,
                      float* voxel_pts, float* voxel_feat, int ldo, int* num_voxels, int* status, void* stream);
/* confidence-quantile mask + row compaction (the voxelize = False branch): threshold = torch.quantile(conf[M], q) ("linear"),
 * rows with conf > threshold are copied in row-major order to out_pts[.][3] / out_feat[.][ldo]; *count_out (device int) = rows kept,
 * *threshold_out (device float) = the quantile.  M <= 2^24.  /root/reference/models/anysplat_stitched.py:381-387, 441-446 */
long v3a_conf_compact_workspace_bytes(long M);
int v3a_conf_quantile_compact(const float* conf, float q, const float* pts, const float* feat, int ldf, int nfeat, long M,
                              void* workspace, long workspace_bytes, float* threshold_out, float* out_pts, float* out_feat, int ldo,
                              int* count_out, void* stream);
/* UnifiedGaussianAdapter + opacity map: feats[U][ldf] = {density logit, 3 scale, 4 quat xyzw, 3*(deg+1)^2 SH}
 * common/gaussian_adapter.py:114-147, common/gaussians.py:33-44, anysplat.py:225-238 (opacity_exponent = 2^x) */
int v3a_gaussian_adapter(const float* pts, const float* feats, int ldf, long U, int sh_degree, float opacity_exponent,
                         const float* sh_mask, float* means, float* cov, float* sh, float* opac, float* scales, float* rot,
                         void* stream);

/* One denoise step's glue between two DiT forwards, as ONE launch: unpatchify of the DiT output tokens, classifier-free guidance,
 * flow-prediction -> x0, UniPC corrector + predictor, and the patchified bf16 input tokens of the next forward.  Replaces the ~25
 * tensor ops of diffusers 0.33.1 `WanPipeline.__call__` (loop body) + `UniPCMultistepScheduler.step` that the reference runs per step
 * (/root/reference/inference_t23d.py:94-103; restated as tensor ops in vist3a_amd/wan/{pipeline,scheduler}.py) with the same
 * rounding points, bit for bit.  The scalar coefficients are the host-side fp32 values `UniPCMultistepScheduler.plan_step` returns. */
typedef struct {
  const void* dit_out;        /* [batch * N][4 C] bf16: DiT output tokens, column (ph * 2 + pw) * C + c; item 0 = conditional, 1 = unconditional */
  void* tok;                  /* [batch * N][4 C] bf16: next forward's input tokens, column c * 4 + ph * 2 + pw (may be NULL) */
  const float* sample;        /* [C][T][H][W] fp32 current latents */
  const float* last_sample;   /* corrected sample of the previous step (corr_order > 0) */
  const float* m_prev1;       /* x0 prediction of the previous step (model_outputs[-1]) */
  const float* m_prev2;       /* ... of the step before (order-2 corrector) */
  float* m_out;               /* this step's x0 prediction */
  float* sample_corrected;    /* corrector output (= sample when corr_order == 0): next step's last_sample */
  float* prev;                /* predictor output: next step's latents */
  int C, T, H, W, batch, guided;
  float guidance, sigma;
  int corr_order;             /* 0 = no corrector (first step), 1, 2 */
  float cc1, cc2, cc3, c_rho_last, c_rho0, c_inv_rk;
  int pred_order;             /* 1, 2 */
  float pc1, pc2, pc3, p_rho0, p_inv_rk;
} v3a_unipc_step_args;
int v3a_unipc_cfg_step(const v3a_unipc_step_args* args, void* stream);
/* fp32 camera-head primitives (vggt/heads/camera_head.py:87-170): y[M<=32][N] = act(x.W^T + b) * gamma + residual */
int v3a_linear_f32(const float* x, const float* w, const float* bias, float* y, const float* residual, const float* gamma,
                   int M, int N, int K, int ldx, int ldy, int ldr, int act, void* stream);
int v3a_attention_small_f32(const float* qkv, float* out, int S, int H, int hd, float scale, void* stream);

/* Skinny GEMM: X has M <= 128 rows, W [N][K] is streamed once (K % 512 == 0).  C[m][n] = act(X.W^T + bias[n]) (+ residual), or the
 * transposed store C[n][m] (bias still indexed by n) for the V^T = Wv.X^T form.  Same rounding points as v3a_gemm_bf16_nt.
 * Replaces nn.Linear on a prompt's tokens: transformers UMT5 q/k/v/o/wi_0/wi_1/wo (the text encoder behind
 * diffusers WanPipeline.encode_prompt; /root/reference/utils/wan_utils.py:25-60). */
typedef struct {
  const void* X; const void* W; void* C;   /* bf16 X, W; C bf16 or fp32 (V3A_GEMM_OUT_F32) */
  const float* bias;                        /* [N] or NULL */
  const void* residual;                     /* C-shaped, bf16 or fp32 (V3A_GEMM_RES_F32), or NULL */
  int M, N, K, ldx, ldw, ldc, ldr;
  int act, flags, transposed_out;
  void* workspace; long workspace_bytes;    /* v3a_gemm_skinny_workspace_bytes(M, N, K) */
} v3a_gemm_skinny_args;
long v3a_gemm_skinny_workspace_bytes(int M, int N, int K);
int v3a_gemm_skinny_bf16(const v3a_gemm_skinny_args* a, void* stream);

/* ---- 3D-Gaussian rasteriser: gsplat==1.4.0 `rasterization(..., render_mode="RGB+D", packed=False,
 * near_plane=1e-10, radius_clip=0.1, covars=..., rasterize_mode="classic")` as driven by
 * third_party_model/anysplat/src/model/decoder/decoder_splatting_cuda.py:96-125.  The reference passes one camera per call;
 * here a call takes C cameras (gsplat's own leading C dimension): per camera the arithmetic is identical, the batch is what
 * fills 256 CUs.  Per-camera arrays are camera-major ([C,U,...], [C,H,W,...]).  All pointers are device pointers unless noted.  Stage 1 = fully_fused_projection + spherical_harmonics (colours only for radii > 0, clamp_min(c + 0.5, 0)). */
typedef struct {
  const float* means;    /* [U,3] world */
  const float* covars;   /* [U,3,3] world covariance, row-major; the upper triangle is used */
  const float* sh;       /* harmonics */
  int sh_layout;         /* 0: [U,K,3] (gsplat argument layout), 1: [U,3,K] (Gaussians.harmonics layout, types.py) */
  int sh_k;              /* K coefficients stored per channel (25) */
  int sh_degree;         /* 0..4 evaluated */
  const float* viewmat;  /* [C,4,4] world->camera, row-major */
  const float* campos;   /* [C,3] camera centre in world = inverse(viewmat)[:3,3] */
  const float* K;        /* [C,3,3] pixel intrinsics */
  long U;
  int C;
  int width, height;
  float near_plane, far_plane, radius_clip, eps2d;
  int* radii;            /* out [C,U]: 3-sigma pixel radius, 0 = culled */
  float* means2d;        /* out [C,U,2] */
  float* depths;         /* out [C,U] camera z */
  float* conics;         /* out [C,U,3] inverse 2D covariance (a,b,c) */
  float* colors;         /* out [C,U,4] rgb + depth */
  int rasterize_mode;    /* 0: classic; 1: antialiased (gsplat rasterize_mode="antialiased", the Mip-Splatting 2D filter); other: -1 */
  float* compensations;  /* out [C,U], mode 1 only (required there: NULL returns -1; ignored in mode 0):
                            sqrt(max(0, det(J Cc J^T) / det(J Cc J^T + eps2d I))), 0 for a culled entry.  Culling, radii, conics,
                            means2d and colours are those of mode 0, bit for bit: gsplat culls and sizes on the blurred covariance. */
} v3a_gs_project_args;
int v3a_gs_project(const v3a_gs_project_args* a, void* stream);

/* Stage 2 = isect_tiles + radix sort by (tile, depth bits) + isect_offset_encode + rasterize_to_pixels (16x16 tiles).
 * Synchronises the stream once (4-byte read-back of the intersection count that sizes the sort, like gsplat's .item()).
 * Returns V3A_ERR_WORKSPACE (-4) when *n_isect > max_isect: call again with a workspace sized for *n_isect. */
typedef struct {
  const int* radii; const float* means2d; const float* depths; const float* conics; const float* colors;
  const float* opacities;   /* [U] (shared by the cameras) */
  const float* background;  /* [3] RGB or NULL (the depth channel's background is 0) */
  long U;
  int C;
  int width, height;
  int clamp_rgb;            /* 1: clamp RGB to [0,1] (decoder_splatting_cuda.py:117) */
  float* out_color;         /* [C,H,W,3] */
  float* out_depth;         /* [C,H,W]  sum(vis_i * z_i) */
  float* out_alpha;         /* [C,H,W]  1 - T */
  void* workspace; long workspace_bytes; long max_isect;
  long* n_isect;            /* HOST pointer: intersections found */
  unsigned int* tile_offsets_out;  /* optional [C*ntiles+1] */
  unsigned int* flatten_ids_out;   /* optional [max_isect]: entry ids c*U+g in composite order */
  const float* compensations;      /* [C,U] of v3a_gs_project (mode 1) or NULL: entry c*U+g draws with opacities[g] * compensations[c*U+g] */
} v3a_gs_rasterize_args;
long v3a_gs_rasterize_workspace_bytes(long U, int C, int width, int height, long max_isect);
int v3a_gs_rasterize(const v3a_gs_rasterize_args* a, void* stream);

/* ---- Backward of the two stages (csrc/raster_bwd.hip): what gsplat's rasterize_to_pixels_bwd, fully_fused_projection_bwd and
 * spherical_harmonics_bwd hand torch.autograd for the call above.  fp32; no float atomics: every sum has a fixed order, so results
 * are bit-identical run to run.  The radius, culling, binning and early-stop decisions of the forward are constants, as in gsplat.
 * Gradients to viewmat / campos (gsplat's optional pose gradients, which the reference's pose optimiser trains through) come from
 * v3a_gs_project_backward_cam only.  NOT computed: the gradient to K (the reference does not optimise intrinsics), cov_ignore=True
 * (quaternion / scale input), packed mode.
 * Antialiased mode (rasterize_mode 1 above): stage 2 differentiates with respect to an entry's EFFECTIVE opacity
 * opacities[g] * compensations[c,g]; stage 1 splits that into the opacity's share and the compensation's, whose gradient
 * d comp / d Sigma2 = ((1 - comp^2) B^-1 - eps2d det(B^-1) I) / (2 comp)  (Sigma2 = J Cc J^T, B = Sigma2 + eps2d I, B^-1 the conic;
 * exactly 0 where comp == 0) joins the conic's before the chain through J, the clamped mean, the rotation and the covariance.
 *
 * Stage 2 backward.  Takes the forward's projected arrays, its composite order (tile_offsets_out / flatten_ids_out and *n_isect of
 * v3a_gs_rasterize) and dL/d(out_color, out_depth, out_alpha); returns the gradient of every camera-Gaussian entry.  Each pixel
 * re-walks its tile list front to back with the forward's arithmetic (same __expf), so it stops where the forward stopped, skips
 * what it skipped (sigma < 0, alpha < 1/255), passes no gradient through an alpha held at the 0.999 cap or a colour clipped by
 * clamp_rgb, and needs neither out_color nor out_alpha.  Workspace: two counters per entry + one 48-byte row per intersection. */
typedef struct {
  const int* radii; const float* means2d; const float* conics; const float* colors;   /* [C,U], [C,U,2], [C,U,3], [C,U,4] */
  const float* opacities;   /* [U] */
  const float* background;  /* [3] or NULL */
  long U;
  int C;
  int width, height;
  int clamp_rgb;
  const unsigned int* tile_offsets;  /* [C*ntiles+1] */
  const unsigned int* flatten_ids;   /* [n_isect] entry ids c*U+g in composite order (may be NULL when n_isect == 0) */
  long n_isect;
  const float* d_color;     /* [C,H,W,3] */
  const float* d_depth;     /* [C,H,W] */
  const float* d_alpha;     /* [C,H,W] */
  float* d_means2d;         /* out [C,U,2] */
  float* d_conics;          /* out [C,U,3] */
  float* d_colors;          /* out [C,U,4] rgb + the depth channel */
  float* d_opacity_partial; /* out [C,U]: this camera's share of dL/d opacities[g] */
  void* workspace; long workspace_bytes;   /* v3a_gs_rasterize_backward_workspace_bytes(U, C, width, height, n_isect); too small: -4 */
  const float* compensations;      /* as v3a_gs_rasterize had it ([C,U] or NULL); d_opacity_partial is then the gradient with
                                      respect to opacities[g] * compensations[c,g] */
  float* d_means2d_abs;     /* out [C,U,2] or NULL: the sum over pixels of |the pixel's two d_means2d terms| (gsplat's absgrad);
                               >= |d_means2d| elementwise, 0 for culled entries.  The other four outputs keep their bits. */
} v3a_gs_rasterize_backward_args;
long v3a_gs_rasterize_backward_workspace_bytes(long U, int C, int width, int height, long max_isect);
int v3a_gs_rasterize_backward(const v3a_gs_rasterize_backward_args* a, void* stream);

/* Stage 1 backward: the entry gradients above -> dL/d(means, covars, sh, opacities), summed over the C cameras in index order.
 * Through the conic (inverse of J Cc J^T + eps2d I), the clamped tx / ty (gradient of min / max as torch takes it), the pixel
 * mean, the depth channel (colors[...,3] = z), the world -> camera rotation of mean and covariance, and the SH colour with its
 * clamp_min(c + 0.5, 0) mask: to the coefficients and, through the normalised view direction, to the means.  Entries with
 * radii == 0 contribute exactly zero.  d_covars follows the forward's "the upper triangle is used": lower-triangle entries are
 * zero, an upper off-diagonal entry carries both symmetric positions.  d_sh has the layout of sh: all sh_k columns are written,
 * bands >= (sh_degree+1)^2 are zero. */
typedef struct {
  const float* means; const float* covars; const float* sh;
  int sh_layout, sh_k, sh_degree;
  const float* viewmat; const float* campos; const float* K;
  long U;
  int C;
  int width, height;
  float eps2d;
  const int* radii;                /* [C,U] of the forward */
  const float* d_means2d; const float* d_conics; const float* d_colors; const float* d_opacity_partial;
  float* d_means;           /* out [U,3] */
  float* d_covars;          /* out [U,3,3] */
  float* d_sh;              /* out, shape and layout of sh */
  float* d_opacities;       /* out [U]; mode 1: sum over c of d_opacity_partial[c,g] * comp[c,g], cameras in index order */
  int rasterize_mode;       /* as v3a_gs_project had it; other than 0 / 1: -1 */
  const float* opacities;   /* [U], mode 1 only (required there: NULL returns -1): dL/dcomp[c,g] = d_opacity_partial[c,g] * opacities[g].
                               comp itself is recomputed from the scene, as everything else here, not read from memory */
} v3a_gs_project_backward_args;
int v3a_gs_project_backward(const v3a_gs_project_backward_args* a, void* stream);

/* Stage 1 backward WITH camera gradients: `a` and its four outputs exactly as above (bit-identical: the same kernel writes them,
 * a second instantiation then evaluates the projection chain again for the camera terms), plus, per camera c with
 * viewmat = [R | t]:   dL/dt = sum_g v_c,   dL/dR = sum_g (v_c m_g^T + 2 W R S_g),   dL/dcampos = -sum_g dL/dd
 * (v_c = the camera-space mean gradient, W = dL/d(R S R^T), d = m_g - campos, the SH view direction; its term is 0 where
 * |d| < 1e-20, as for the means).  d_viewmat [C,4,4]: all 16 entries written, the bottom row as zeros; d_campos [C,3].  No float
 * atomics: every entry's 15 fp32 terms are converted (exactly) to fp64, summed over the wave of 64 Gaussians in a fixed order
 * into one partial row of `workspace` ([C, ceil(U / 64), 15] doubles, 8-byte aligned), and a second launch adds each camera's
 * rows in a fixed order and rounds ONCE to fp32.  Entries with radii == 0 contribute exact zeros.  Too small a workspace: -4.
 * `workspace` must be a non-null, 8-byte aligned pointer even for U == 0, where the queried size is 0 and nothing is read (-1
 * otherwise): with U == 0 the outputs are written as exact zeros. */
long v3a_gs_project_backward_cam_workspace_bytes(long U, int C);   /* V3A_ERR_SHAPE for U < 0, U >= 2^31 or C < 1 */
int v3a_gs_project_backward_cam(const v3a_gs_project_backward_args* a, float* d_viewmat, float* d_campos, void* workspace,
                                long workspace_bytes, void* stream);

/* ---- Image-pair metrics of the novel-view-synthesis evaluation (calculate_metric.py; anysplat/src/evaluation/metrics.py:11-55):
 * per pair, SSIM as skimage.metrics.structural_similarity(win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0)
 * computes it, and the MSE of compute_psnr (PSNR = -10 log10(mse) on the host), both on uint8 / 255 in fp32 (PNG pixels read back
 * with ToTensor).  One call = two launches; fp64 partials reduced in a fixed order (bit-identical run to run, no atomics).
 * H, W >= 11 (skimage's minimum for win_size 11), 1 <= C <= 4. */
typedef struct {
  const uint8_t* a;         /* [N,H,W,C] uint8 (PNG byte order) */
  const uint8_t* b;         /* [N,H,W,C] uint8 */
  int N, H, W, C;
  double* ssim;             /* out [N] */
  double* mse;              /* out [N] */
  void* workspace; long workspace_bytes;   /* v3a_image_metrics_workspace_bytes(N, H, W, C) */
} v3a_image_metrics_args;
long v3a_image_metrics_workspace_bytes(int N, int H, int W, int C);   /* V3A_ERR_SHAPE for a shape the metric rejects */
int v3a_image_metrics(const v3a_image_metrics_args* a, void* stream);

/* ---- LPIPS(VGG) of the novel-view-synthesis evaluation (calculate_metric.py; anysplat/src/evaluation/metrics.py:22-34, lpips 0.1
 * `LPIPS(net="vgg")` with normalize=True).  The 13 VGG-16 convolutions are v3a_conv_split (act RELU, pair output); these are the passes
 * around them (csrc/lpips.hip).  A pair tensor is two bf16 planes (hi, lo) of the same shape, channels-last.
 *   v3a_lpips_input   pred, gt: uint8 [N,H,W,3] (f32_nchw = 0) or f32 [N,3,H,W] in [0,1] (f32_nchw = 1) -> y planes [2N][H][W][CinP]
 *                     (frames [0,N) = pred, [N,2N) = gt; CinP 8 or 16, channels 3.. zero): fp32 x = u / 255, 2 x - 1, (x - shift) / scale
 *                     (lpips ScalingLayer), each step rounded as torch rounds it, then split (hi, lo).  2N <= 65535.
 *   v3a_lpips_pool    nn.MaxPool2d(2, 2), floor mode, on pair planes [F][H][W][C] -> [F][H/2][W/2][C] (C % 8 == 0): (hi, lo) compared
 *                     lexicographically, the winner copied verbatim.
 *   v3a_lpips_head    one tapped layer, planes [2N][h][w][C] (C = 8 * 2^k <= 512), lin weight f32 [C]: per pixel f = hi + lo,
 *                     f^ = f / (sqrt(sum_c f^2) + 1e-10), d = sum_c w[c] (f^_pred - f^_gt)^2 in fp64; out[n] = mean of d over h x w
 *                     (accumulate != 0: added to out[n]).  Two launches, fp64 partials reduced in a fixed order that depends on
 *                     (h, w, C) only: bit-identical run to run and for any N.  workspace: v3a_lpips_head_workspace_bytes(N, h, w, C)
 *                     (V3A_ERR_SHAPE for a shape the head rejects). */
int v3a_lpips_input(const void* pred, const void* gt, int f32_nchw, int N, int H, int W, int CinP, void* y_hi, void* y_lo, void* stream);
int v3a_lpips_pool(const void* x_hi, const void* x_lo, void* y_hi, void* y_lo, int F, int H, int W, int C, void* stream);
long v3a_lpips_head_workspace_bytes(int N, int h, int w, int C);
int v3a_lpips_head(const void* x_hi, const void* x_lo, const float* weight, int N, int h, int w, int C, double* out, int accumulate,
                   void* workspace, long workspace_bytes, void* stream);

/* ---- CLIP score of the generated-scene evaluation (evaluation/gen_eval/t3_scene_evaluation.py:97-120 of the reference: torchmetrics
 * CLIPScore on a Hugging Face CLIPModel).  The towers' linear layers are v3a_conv_split (1x1, act QUICK_GELU for fc1), their LayerNorms
 * v3a_layernorm / v3a_layernorm_pair; these are the passes around them (csrc/clip.hip).
 *   v3a_clip_preprocess  CLIPImageProcessor on the Pillow path for N uint8 frames [N,H,W,3]: BICUBIC resize exactly as Pillow's
 *                        ImagingResample does it for 8-bit channels (horizontal pass, rounded and clipped to uint8, then vertical pass; per
 *                        output sample clip8(((1 << 21) + sum k_i p_i) >> 22)), the centre crop to S x S, the value table lut [3][256]
 *                        (rescale and normalise in fp32, built by the host) and the patch matrix [N (S/P)^2][ldk] as a (hi, lo) pair:
 *                        column c P^2 + py P + px, columns 3 P^2 .. ldk zero (ldk % 8 == 0).  The host passes, for the S kept columns and
 *                        the S kept rows, Pillow's bounds [S][2] (first input sample, tap count) and 22-bit fixed-point coefficients
 *                        [S][kx] / [S][ky], and the input rows the vertical taps read: row0 .. row0 + rows.  Every bound must lie inside
 *                        the image / that row range - the tables live on the device, so this entry point CANNOT check them: a caller
 *                        with mismatched tables reads out of bounds (vist3a_amd.ops.clip_preprocess checks them on the host).  out_u8 [N,S,S,3] and out_f32 [N,3,S,S] are optional copies of the crop.
 *                        workspace: v3a_clip_preprocess_workspace_bytes(N, rows, S).
 *   v3a_clip_rows        token assembly, f32 rows of d (d % 4 == 0): out[r] = src[row(r)] + pos[r % S] (pos may be NULL), r < M;
 *                        row(r) = ids[r] (clamped to src_rows) when ids is given; else with cls given the class token at r % S == 0 and
 *                        src row r - r / S - 1 elsewhere (src = [M / S][S - 1][d]); else r.
 *   v3a_attention_f32    softmax(scale q k^T) v in fp32 for B sequences of S <= 1024 rows and H heads of hd = 64 (any other hd:
 *                        V3A_ERR_SHAPE).  q, k, v: f32, row b S + s at stride ld, head h at column 64 h.  causal != 0 masks keys > query;
 *                        lens [B] (or NULL) masks keys >= lens[b].  Output row stride ldo: f32 (o_f32) and / or a (hi, lo) pair.  Products
 *                        and the softmax accumulate in fp32, a row's keys in index order on one lane: bit-reproducible, independent of B.
 *   v3a_clip_score       fp64: scores[f] = max(100 cos(image_emb[f], text_emb), 0), f < F, embeddings f32 of D; *mean (may be NULL) =
 *                        their mean, summed in frame order.  A zero embedding gives NaN, as torchmetrics does.  One workgroup, no atomics. */
typedef struct {
  const void* src;
  const int* x_bounds; const int* x_coeffs; const int* y_bounds; const int* y_coeffs;
  const float* lut;
  void* patches_hi; void* patches_lo;
  void* out_u8; float* out_f32;
  int N, H, W, S, P, ldk, kx, ky, row0, rows;
  void* workspace; long workspace_bytes;
} v3a_clip_preprocess_args;
long v3a_clip_preprocess_workspace_bytes(int N, int rows, int S);
int v3a_clip_preprocess(const v3a_clip_preprocess_args* args, void* stream);
int v3a_clip_rows(const float* src, int src_rows, const int* ids, const float* cls, const float* pos, float* out, long M, int S, int d,
                  void* stream);
int v3a_attention_f32(const float* q, const float* k, const float* v, int ld, void* o_hi, void* o_lo, float* o_f32, int ldo,
                      const int* lens, int B, int S, int H, int hd, float scale, int causal, void* stream);
int v3a_clip_score(const float* image_emb, const float* text_emb, int F, int D, double* scores, double* mean, void* stream);

/* ---- Post-optimisation of predicted Gaussians (third_party_model/anysplat/src/post_opt/simple_trainer.py; vist3a_amd/post_opt).
 *
 * Photometric loss (csrc/ssim_loss.hip): pred, target f32 [N,H,W,C] (the rasteriser's layout), C <= 4, H, W >= 11 (smaller:
 * V3A_ERR_SHAPE; the reference would silently skip the smoothing).  out[0] = loss = (1 - ssim_lambda) l1 + ssim_lambda (1 - ssim),
 * out[1] = l1 = mean |pred - target|, out[2] = ssim = mean over the (H-10) x (W-10) valid map, all channels and images, of the
 * reference's loss_ssim.py::ssim(data_range=1.0) (11-tap Gaussian, sigma 1.5, population variances, C1 = 1e-4, C2 = 9e-4).  fp64
 * arithmetic on the fp32 inputs; fp64 partials reduced in a fixed order: bit-identical run to run; identical images give exactly
 * (0, 0, 1).  Forward = two launches; with planes != NULL it also stores the three derivative planes [3][N][C][H-10][W-10] (fp64)
 * that the backward reads.  Backward = one launch, gather form, no atomics: d_pred (f32, shape of pred, every element written
 * once) from d_out[3] = the gradients of (loss, l1, ssim) on the device; sign(0) = 0 in the L1 part. */
typedef struct {
  const float* pred; const float* target;
  int N, H, W, C;
  double ssim_lambda;
  double* out;                               /* [3]: loss, l1, ssim (forward only) */
  void* workspace; long workspace_bytes;     /* v3a_photometric_loss_workspace_bytes(N, H, W, C) (forward only) */
  double* planes; long planes_bytes;         /* v3a_photometric_loss_planes_bytes(N, H, W, C); NULL in a forward without gradient */
} v3a_photometric_loss_args;
long v3a_photometric_loss_workspace_bytes(int N, int H, int W, int C);   /* V3A_ERR_SHAPE for a shape the loss rejects */
long v3a_photometric_loss_planes_bytes(int N, int H, int W, int C);
int v3a_photometric_loss_forward(const v3a_photometric_loss_args* a, void* stream);
int v3a_photometric_loss_backward(const v3a_photometric_loss_args* a, const double* d_out, float* d_pred, void* stream);

/* Depth term (csrc/depth_loss.hip; simple_trainer.py:943-961 with `points` = the integer coordinates of the used pixels): depth, alpha
 * f32 [C,H,W] as v3a_gs_rasterize emits them (depth = the alpha-weighted z), depth_gt f32 [C,H,W], mask uint8 [C,H,W] (nonzero = use
 * the pixel) or NULL (all), C H W < 2^31.  Per pixel in fp64: E = depth / max(alpha, 1e-10) (gsplat's expected depth, never
 * materialised), disp = E > 0 ? 1 / E : 0, used = mask && depth_gt > 0 && isfinite(depth_gt), term = |disp - 1 / depth_gt|;
 * out[0] = loss = scale * sum(term) / M, out[1] = M = the number of used pixels of all C cameras.  Deviations from the reference: a
 * pixel whose target is not a positive finite number is skipped (the reference divides by it), and M == 0 gives loss 0 and zero
 * gradients (the reference's empty mean is NaN).  Forward = two launches, fp64 partials and integer counts per workgroup reduced in a
 * fixed order: bit-identical run to run, no atomics.  Backward = one launch: d_depth, d_alpha (f32 [C,H,W], every element written
 * once, zero where the pixel is unused or E <= 0) from d_out[1] = the gradient of loss on the device; it reads M from `out` as the
 * forward left it (on the device), is exactly linear in d_out, and takes sign(0) = 0.  16-byte accesses where depth, alpha,
 * depth_gt (and d_depth, d_alpha) are 16-byte and mask 4-byte aligned, scalar otherwise. */
typedef struct {
  const float* depth; const float* alpha; const float* depth_gt;
  const unsigned char* mask;                 /* or NULL */
  int C, H, W;
  double scale;                              /* the reference's scene_scale */
  double* out;                               /* [2]: loss, M (written by the forward, read by the backward) */
  void* workspace; long workspace_bytes;     /* v3a_depth_loss_workspace_bytes(C, H, W), 8-byte aligned (forward only) */
} v3a_depth_loss_args;
long v3a_depth_loss_workspace_bytes(int C, int H, int W);   /* V3A_ERR_SHAPE for a non-positive or too large size */
int v3a_depth_loss_forward(const v3a_depth_loss_args* a, void* stream);
int v3a_depth_loss_backward(const v3a_depth_loss_args* a, const double* d_out, float* d_depth, float* d_alpha, void* stream);

/* Bilateral-grid colour compensation (csrc/bilagrid.hip; lib_bilagrid.py::BilateralGrid / slice / total_variation_loss, one grid per
 * image): rgb f32 [N,H,W,3], grids f32 [N,L,GY,GX,12] coefficient-minor (coefficient 4c + k = row c, column k of the 3x4 matrix),
 * GX, GY, L >= 2 (smaller: V3A_ERR_SHAPE; the reference degenerates silently), N H W 3 and N L GY GX 12 < 2^31.  Per pixel (i, j) in
 * fp64: x = (j + 0.5) / W, y = (i + 0.5) / H, gray = 0.299f r + 0.587f g + 0.114f b; the grid is sampled as
 * grid_sample(bilinear, align_corners=True, border) at (x (GX-1), y (GY-1), clamp(gray (L-1), 0, L-1)) and
 * out[c] = A[c][0] r + A[c][1] g + A[c][2] b + A[c][3], rounded to f32 once.  Backward: d_rgb (through the matrix and through the
 * guidance coordinate, whose term is exactly 0 where gray (L-1) <= 0 or >= L-1) and d_grids (a gather, one workgroup per vertex,
 * fixed-order reduction, no atomics: every element written exactly once, zeros included); either may be NULL.  Both are
 * bit-identical run to run and exactly linear in d_out. */
typedef struct {
  const float* rgb; const float* grids;
  int N, H, W;
  int GX, GY, L;
} v3a_bilagrid_slice_args;
int v3a_bilagrid_slice_forward(const v3a_bilagrid_slice_args* a, float* out, void* stream);
int v3a_bilagrid_slice_backward(const v3a_bilagrid_slice_args* a, const float* d_out, float* d_rgb, float* d_grids, void* stream);

/* Total variation of grids f32 [V,L,GY,GX,12] (total_variation_loss): for each of the axes L, GY, GX the sum of squared forward
 * differences over 12 * (L GY GX with that axis' size - 1), added and divided by V -> out[0] (fp64).  Forward = two launches, fp64
 * partials per workgroup reduced in a fixed order.  Backward = one launch, d_grids (f32, every element written once) from
 * d_out[1] on the device, exactly linear in it. */
typedef struct {
  const float* grids;
  int V, GX, GY, L;
  double* out;                               /* [1] (forward only) */
  void* workspace; long workspace_bytes;     /* v3a_bilagrid_tv_workspace_bytes(V, GX, GY, L), 8-byte aligned (forward only) */
} v3a_bilagrid_tv_args;
long v3a_bilagrid_tv_workspace_bytes(int V, int GX, int GY, int L);   /* V3A_ERR_SHAPE for a size under 2 or too large */
int v3a_bilagrid_tv_forward(const v3a_bilagrid_tv_args* a, void* stream);
int v3a_bilagrid_tv_backward(const v3a_bilagrid_tv_args* a, const double* d_out, float* d_grids, void* stream);

/* Colour correction before PSNR (csrc/color_correct.hip; lib_bilagrid.py:56-126 color_correct, the cc_psnr of simple_trainer.py::eval).
 * img, ref, out: f32 [N,H,W,3], a pixel's three channels contiguous, row stride ld_* and image stride *_stride in ELEMENTS
 * (ld >= 3 W, stride >= (H - 1) ld + 3 W for N > 1: V3A_ERR_SHAPE otherwise); only the [H, 3 W] region of each image is read or
 * written.  Per image, num_iters (1 .. 16) rounds on the estimate x (= img at first, not clipped): features
 * (r^2, rg, rb, g^2, gb, b^2, r, g, b, 1) of x; for each output channel c the least-squares fit of the 10 coefficients to ref[c]
 * over the pixels with img[c], x[c] and ref[c] all in [eps, 1 - eps]; x = clip(features . warp, 0, 1).  fp64 after the f32 loads
 * (sums, the 10 x 10 normal equations solved on the device, the update); out is rounded to f32 once and every element of it is
 * written exactly once.  sse[n] = sum over the image of (out - ref)^2 in fp64, of the stored f32 values.
 * status[n][c] (a deviation: the reference asserts or is undefined on such a channel): bit 0 = in some round fewer than 10 pixels
 * were usable, bit 1 = a pivot of the elimination was <= 1e-12 times its diagonal entry of the Gram matrix (or the solution was
 * not finite); in such a round the channel keeps the identity warp (x[c] passes through, clipped).  0 = every round was solved.
 * 2 num_iters + 2 launches, fixed-order reductions, no atomics: bit-identical run to run, and an image's result does not depend
 * on the other images of the call.  0 <= eps < 0.5 (V3A_ERR_ARG otherwise); float pointers 4-byte, sse 8-byte aligned (V3A_ERR_ARG). */
typedef struct {
  const float* img; const float* ref;
  float* out;
  int N, H, W;
  int num_iters;
  long ld_img, ld_ref, ld_out;                /* row strides, elements */
  long img_stride, ref_stride, out_stride;    /* image strides, elements (unused for N = 1) */
  double eps;
  double* sse;                                /* out [N] */
  int32_t* status;                            /* out [N,3] */
  void* workspace; long workspace_bytes;      /* v3a_color_correct_workspace_bytes(N, H, W, num_iters), 8-byte aligned */
} v3a_color_correct_args;
long v3a_color_correct_workspace_bytes(int N, int H, int W, int num_iters);   /* V3A_ERR_SHAPE for a size the fit rejects */
int v3a_color_correct(const v3a_color_correct_args* a, void* stream);

/* Plain per-image mean squared error of two f32 images [N,H,W,C] (csrc/color_correct.hip), rows of W C contiguous elements at
 * row stride ld_*, images at *_stride (elements, as above): mse[n] = sum (a - b)^2 / (H W C), the difference and the sum in fp64,
 * workgroup partials reduced in a fixed order (two launches, no atomics).  PSNR = -10 log10(mse) is the caller's. */
typedef struct {
  const float* a; const float* b;
  int N, H, W, C;
  long ld_a, ld_b;
  long a_stride, b_stride;
  double* mse;                                /* out [N] */
  void* workspace; long workspace_bytes;      /* v3a_image_mse_workspace_bytes(N, H, W, C), 8-byte aligned */
} v3a_image_mse_args;
long v3a_image_mse_workspace_bytes(int N, int H, int W, int C);   /* V3A_ERR_SHAPE for a non-positive or too large size */
int v3a_image_mse(const v3a_image_mse_args* a, void* stream);

/* Splat activation (csrc/post_opt.hip), one thread per Gaussian: log-scales [U,3], raw quaternions [U,4] (xyzw, any length),
 * opacity logits [U] -> covariances [U,3,3] = R diag(exp(log_scale))^2 R^T with v3a_gaussian_adapter's quaternion order,
 * normalisation and product, opacities [U] = sigmoid.  Backward: closed form from (d_covars, d_opacities); d_covars is contracted
 * entry by entry, so the upper-triangle convention of v3a_gs_project_backward and a full symmetric gradient both give what autograd
 * through the product gives. */
int v3a_splat_activate(const float* log_scales, const float* quats, const float* logits, long U, float* covars, float* opacities,
                       void* stream);
int v3a_splat_activate_backward(const float* log_scales, const float* quats, const float* logits, const float* d_covars,
                                const float* d_opacities, long U, float* d_log_scales, float* d_quats, float* d_logits, void* stream);

/* Fused Adam (csrc/post_opt.hip), one launch per parameter tensor, in place on p, m, v (f32 [n]), reading g:
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;  p -= lr / bias_correction1 * m / (sqrt(v) / sqrt(bias_correction2) + eps)
 * (torch.optim.Adam; the bias corrections 1 - beta^t come from the host in double).  period > 0: element e uses lr when
 * e % period == 0 and lr2 otherwise (harmonics [U,3,K] with period K: the DC band and the rest are the reference's two optimisers);
 * period == 0: lr everywhere.  16-byte loads and stores with a scalar tail (all scalar when a pointer is not 16-byte aligned). */
typedef struct {
  float* p; const float* g; float* m; float* v;
  long n;
  double lr, lr2;
  int period;
  double beta1, beta2, eps, bias_correction1, bias_correction2;
} v3a_adam_args;
int v3a_adam_step(const v3a_adam_args* a, void* stream);

/* The step's visibility mask (csrc/post_opt.hip; simple_trainer.py:1111, (info["radii"] > 0).any(0)): radii int32 [C,U] as
 * v3a_gs_project writes them -> visible uint8 [U], 1 where radii[c,g] > 0 for some camera c, else 0.  One thread per Gaussian,
 * the cameras walked in index order; every output byte is written exactly once (no atomics, no memset).  C >= 1, U >= 1. */
int v3a_gs_visibility(const int* radii, int C, long U, uint8_t* visible, void* stream);

/* Visibility-masked Adam (csrc/post_opt.hip; gsplat's SelectiveAdam, simple_trainer.py:449-450), one launch per parameter tensor:
 * p, g, m, v are f32 [U, M] (M floats per row), visible uint8 [U].  For every row with visible != 0 and every element of it
 *   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;  p -= lr * m / (sqrt(v) + eps)
 * with NO bias correction (there is no step argument).  A row with visible == 0 is not touched: its p, m, v are neither loaded
 * nor stored and its g is NOT LOADED (a NaN there cannot reach a result) - the rows the mask clears belong to the caller, as the
 * memory contract above says of skipped rows.  period / lr2 as in v3a_adam_step, the element index e taken within the whole
 * tensor.  Arithmetic as v3a_adam_step: fp64 after the loads, one rounding at each store.  Thread t owns elements 4t .. 4t + 3
 * of the flat tensor: 16-byte loads and stores where all four lie in visible rows, element by element where a visible and an
 * invisible row meet, nothing where none is visible; a scalar tail (all scalar when a pointer is not 16-byte aligned). */
typedef struct {
  float* p; const float* g; float* m; float* v;
  const uint8_t* visible;
  long U; long M;
  double lr, lr2;
  int period;
  double beta1, beta2, eps;
} v3a_adam_visible_args;
int v3a_adam_step_visible(const v3a_adam_visible_args* a, void* stream);

/* The pose optimiser's parametrisation (csrc/post_opt.hip; post_opt/utils.py:12-48 CameraOptModule, :117-138): per camera 9
 * deltas (dx[3], drot[6]); a1 = drot[0..2] + (1,0,0), a2 = drot[3..5] + (0,1,0), b1 = a1 / max(|a1|, 1e-12),
 * b2 = normalise(a2 - (b1 . a2) b1) with the same clamp, b3 = b1 x b2, Rd = the matrix with ROWS b1, b2, b3, and the adjusted
 * camera is c2w' = c2w_base [Rd | dx].  What the rasteriser takes follows in closed form from the base matrices [V,4,4]:
 *   viewmat [V,4,4] = inverse(c2w') = [Rd^T | -Rd^T dx] w2c_base,     campos [V,3] = c2w'[:3,3] = c2w_base[:3,:3] dx + c2w_base[:3,3].
 * One thread per camera, fp64 after the loads, one rounding at the store; zero deltas return the base matrices bit for bit
 * (every product is by exactly 1 or 0).  Backward: (d_viewmat [V,4,4], d_campos [V,3]) -> d_deltas [V,9], closed form through
 * the product and the Gram-Schmidt steps, every element written once, exactly linear in the incoming gradients; the bottom row
 * of d_viewmat is not read (viewmat's is the base's).  1 <= V <= 2^24 (V3A_ERR_SHAPE otherwise). */
int v3a_camera_adjust(const float* w2c_base, const float* c2w_base, const float* deltas, int V, float* viewmat, float* campos,
                      void* stream);
int v3a_camera_adjust_backward(const float* w2c_base, const float* c2w_base, const float* deltas, const float* d_viewmat,
                               const float* d_campos, int V, float* d_deltas, void* stream);

/* The post-optimisation loop's two regularisers (csrc/splat_reg.hip; simple_trainer.py:966-977): from opacity logits f32 [U] and
 * log-scales f32 [U,3], out f64 [2] = (mean sigmoid(logit), mean exp(log_scale)) - the reference's abs() is the identity on both.
 * fp64 after the loads; one partial pair per workgroup of a grid fixed by U, then a one-workgroup reduction in the order of
 * csrc/fixed_sum.h: no atomics, bit-identical run to run.  workspace: v3a_splat_reg_workspace_bytes(U), 8-byte aligned (too small
 * or misaligned: -4).  Backward (elementwise, every element written once, exactly linear in d_out f64 [2] on the device):
 *   d_logits[i] = d_out[0] s (1 - s) / U,   d_log_scales[i] = d_out[1] exp(log_scale) / (3 U).
 * 16-byte loads and stores with a scalar tail (all scalar for an array whose pointers are not 16-byte aligned). */
long v3a_splat_reg_workspace_bytes(long U);   /* V3A_ERR_SHAPE for U < 1 or 3 U > 2^31 - 1 */
int v3a_splat_reg(const float* logits, const float* log_scales, long U, double* out, void* workspace, long workspace_bytes, void* stream);
int v3a_splat_reg_backward(const float* logits, const float* log_scales, long U, const double* d_out, float* d_logits,
                           float* d_log_scales, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The MCMC strategy of the post-optimisation loop (csrc/mcmc.hip; gsplat's MCMCStrategy, which simple_trainer.py:1142-1150 calls
 * in its `mcmc` configuration).  DESIGN.md section 7f restates the algorithm and is the contract.
 *
 * Random numbers: Philox4x32-10, counter (slot, 0, rng_stream, step), key = seed (low word, high word); no state.  rng_stream 0 is
 * relocation sampling, 1 growth sampling, 2 and 3 the two normal draws of the noise, 4 to 7 those of v3a_densify_apply's split children.  A uniform of words (x0, x1) is
 * ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53 in [0, 1).  v3a_mcmc_philox and v3a_mcmc_uniform run on the HOST (host pointers): the same
 * source as the device code, for known-answer tests.
 * ---------------------------------------------------------------------------------------------- */
int v3a_mcmc_philox(const uint32_t* counter /* [4] */, const uint32_t* key /* [2] */, uint32_t* out /* [4] */);
double v3a_mcmc_uniform(uint32_t x0, uint32_t x1);

/* Weighted sampler.  weights f32 [U] (opacities); src int32 [n_slots]; counts int32 [U], zeroed by the call, then counts[src[s]] += 1
 * for every slot that drew (integer atomics: they commute).
 *   alive_only = 1 (relocation): n_slots == U; slot s is active iff weights[s] <= min_weight, inactive slots get src = -1; the pool is
 *                                weights[i] where above min_weight, else 0.
 *   alive_only = 0 (growth):     every slot is active, the pool is all weights; min_weight is ignored.
 * All sums in fp64 on the exactly converted weights: blocks of 1024 consecutive Gaussians, block total T_b = each of 256 lanes adds
 * its 4 consecutive elements in index order, then block_sum<256> of csrc/fixed_sum.h; P_b = the exclusive prefix of T_b added
 * sequentially in block order, total = P_last + T_last.  An active slot draws t = u total, takes b = the last block with T_b > 0 and
 * P_b <= t, walks it in index order (c = P_b; c += w_i) and picks the first i with w_i > 0 and c > t, or else the block's last i
 * with w_i > 0.  total == 0 or no active slot: every src is -1, every count 0, no error.  Nothing is read back to the host.
 * workspace: v3a_mcmc_sample_workspace_bytes(U), 8-byte aligned (too small or misaligned: -4). */
long v3a_mcmc_sample_workspace_bytes(long U);   /* V3A_ERR_SHAPE for U < 1 or U > 2^31 - 1 */
int v3a_mcmc_sample(const float* weights, long U, float min_weight, int alive_only, long n_slots, unsigned long long seed,
                    unsigned int rng_stream, unsigned int step, int* src, int* counts, void* workspace, long workspace_bytes, void* stream);

/* Relocation (dst_offset == 0, n_slots == U: slot s is row s, a dead row) and growth (dst_offset == U: slot s is row U + s of
 * tensors the caller allocated with U + n_slots rows and filled up to U), from the sampler's src and counts.  For a source j
 * (counts[j] > 0), in fp64 with one rounding per f32 store:
 *   r = min(counts[j] + 1, 51), op = sigmoid(logit_j), o' = 1 - (1 - op)^(1/r),
 *   den = sum_{i=1..r} sum_{k=0..i-1} C(i-1, k) (-1)^k / sqrt(k+1) o'^(k+1),  scale' = (op / den) exp(log_scale_j),
 *   stored: logit(clamp(o', min_opacity, 1 - 2^-23)) and log(scale').
 * Row j takes the new logit and log-scales; the row of every slot with src == j takes them too, with means, quats and sh of row j.
 * Moments: relocation zeroes m and v of row j in all five tensors and leaves the dead row's; growth zeroes the new row's and leaves
 * row j's.  Per-source values go to the workspace first, then every row is written by exactly one thread: the result does not
 * depend on execution order.  Rows that are neither source nor destination are not touched.  src and counts must be one
 * v3a_mcmc_sample's output (a slot whose src is out of range or has counts 0 is skipped).
 * workspace: v3a_mcmc_relocate_workspace_bytes(U) (16 U), 8-byte aligned. */
typedef struct {
  const int* src;      /* [n_slots] */
  const int* counts;   /* [U] */
  float *means, *log_scales, *quats, *logits, *sh;            /* [rows,3] [rows,3] [rows,4] [rows] [rows,3,K]; rows = U or U + n_slots */
  float *m_means, *m_log_scales, *m_quats, *m_logits, *m_sh;  /* Adam's first moments, same shapes */
  float *v_means, *v_log_scales, *v_quats, *v_logits, *v_sh;  /* Adam's second moments */
  long U, n_slots, dst_offset;
  int K;
  double min_opacity;                         /* in (0, 1) */
  void* workspace; long workspace_bytes;
} v3a_mcmc_relocate_args;
long v3a_mcmc_relocate_workspace_bytes(long U);   /* V3A_ERR_SHAPE for U < 1 or U > 2^31 - 1 */
int v3a_mcmc_relocate(const v3a_mcmc_relocate_args* a, void* stream);

/* The per-step noise, in place on means f32 [U,3], one thread per Gaussian, fp64 after the loads, one rounding at the store:
 *   op = sigmoid(logit), gate = 1 / (1 + exp(-100 ((1 - op) - 0.995))), cov = R diag(exp(2 log_scale)) R^T with R from the raw
 *   quaternion by v3a_splat_activate's expression (evaluated in fp64), xi = (z0, z1) of rng_stream 2 and z0 of rng_stream 3 at
 *   slot i (Box-Muller: r = sqrt(-2 ln(1 - u1)), z0 = r cos(2 pi u2), z1 = r sin(2 pi u2), u1 from words 0-1, u2 from words 2-3),
 *   means_i += cov (xi gate scaler).
 * 44 bytes read and 12 written per Gaussian; the quaternion is one 16-byte load when its pointer is 16-byte aligned. */
int v3a_mcmc_noise(float* means, const float* log_scales, const float* quats, const float* logits, long U, double scaler,
                   unsigned long long seed, unsigned int step, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Adaptive density control of the post-optimisation loop (csrc/densify.hip; gsplat's DefaultStrategy, which the reference's
 * `default` configuration is built around, simple_trainer.py:1486-1491).  DESIGN.md section 7f restates it and is the contract.
 * Shape rules of all four: U < 0 or U >= 2^31 returns V3A_ERR_SHAPE, U == 0 is a no-op.
 *
 * Accumulate (every step): for Gaussian g and every camera c in index order with radii[c,g] > 0,
 *   s += sqrt((gx W/2 C)^2 + (gy H/2 C)^2) in fp64, (gx, gy) = d_means2d[c,g]; n += 1;
 * then grad2d[g] = (float)(grad2d[g] + s) - one rounding per call - and count[g] += n.  One thread per Gaussian, no scratch. */
int v3a_densify_accumulate(const float* d_means2d /* [C,U,2] */, const int* radii /* [C,U] */, long U, int C, int width, int height,
                           float* grad2d /* [U] */, int* count /* [U] */, void* stream);

/* Classify (every refine).  Per parent g, in fp64 on exactly converted f32 values:
 *   high = grad2d / max(count, 1) > grow_grad2d;  small = max_k exp(ls[g,k]) <= grow_scale3d
 *   fate = grow ? (high ? (small ? CLONE : SPLIT) : KEEP) : KEEP                       (0 keep, 1 clone, 2 split)
 *   the rows it leaves are a keep's or clone's copies of the parent (opacity o = sigmoid(logit), scale smax) or a split's two
 *   children (opacity o, or 1 - sqrt(1 - o) with revised_opacity; scale smax / 1.6); they share one verdict:
 *   pruned = opacity < prune_opa || (prune_big && scale > prune_scale3d)
 *   fates[g] = fate | pruned << 2
 *   counts[0][g] = fate != SPLIT && !pruned   (segment A: the original)
 *   counts[1][g] = fate == CLONE && !pruned   (segment B: the clone)
 *   counts[2][g] = fate == SPLIT && !pruned   (segments C and D: the first and the second child)
 * offsets[s] is the exclusive prefix sum of counts[s] (blocks of 256 parents, then the block totals in order: integers, so the
 * order cannot change the result) and totals[s] its sum, int64 [3] on the device.  The thresholds come multiplied by the scene
 * scale.  workspace: v3a_densify_classify_workspace_bytes(U), 8-byte aligned (too small or misaligned: V3A_ERR_WORKSPACE). */
typedef struct {
  const float* grad2d; const int* count;          /* [U] */
  const float* log_scales; const float* logits;   /* [U,3], [U] */
  long U;
  double grow_grad2d, grow_scale3d, prune_opa, prune_scale3d;
  int grow, prune_big, revised_opacity;
  unsigned char* fates;   /* out [U] */
  int* counts;            /* out [3,U] */
  int* offsets;           /* out [3,U] */
  long* totals;           /* out [3], device */
  void* workspace; long workspace_bytes;
} v3a_densify_classify_args;
long v3a_densify_classify_workspace_bytes(long U);   /* V3A_ERR_SHAPE for U < 0 or U >= 2^31 */
int v3a_densify_classify(const v3a_densify_classify_args* a, void* stream);

/* Apply (every refine): the new tensors of U_out = totals[0] + totals[1] + 2 totals[2] rows, from the old ones and classify's
 * fates, offsets and totals.  Row order: A surviving non-split originals in index order (row offsets[0][g]), B surviving clones
 * (totals[0] + offsets[1][g]), C first children (totals[0] + totals[1] + offsets[2][g]), D second children (C's base + totals[2]
 * + offsets[2][g]).  A rows copy the parent and its moments bit for bit; a B row copies the parent with zero moments; child c of a
 * split has ls - log 1.6, the parent's logit (or logit(1 - sqrt(1 - o)) with revised_opacity), quats and sh, zero moments and
 *   means + R (exp(ls) . z),  R = quat_R of csrc/splat_quat.h, z = (z0, z1) of rng_stream 4 + 2c and z0 of rng_stream 5 + 2c of
 * v3a_mcmc_philox at counter (g, 0, rng_stream, step), key = seed (Box-Muller as for v3a_mcmc_noise); fp64, one rounding per store.
 * Every element of every new tensor is written exactly once, zeros included; no memset, no atomics.  A row past U_out is not
 * written.  The harmonics rows move with 16-byte accesses where source and destination share their phase, scalar otherwise.
 * Old and new tensors must not overlap (V3A_ERR_SHAPE).  U_out == 0 writes nothing. */
typedef struct {
  const float *means, *log_scales, *quats, *logits, *sh;            /* old: [U,3] [U,3] [U,4] [U] [U,3,K] */
  const float *m_means, *m_log_scales, *m_quats, *m_logits, *m_sh;
  const float *v_means, *v_log_scales, *v_quats, *v_logits, *v_sh;
  float *new_means, *new_log_scales, *new_quats, *new_logits, *new_sh;   /* new: U_out rows */
  float *new_m_means, *new_m_log_scales, *new_m_quats, *new_m_logits, *new_m_sh;
  float *new_v_means, *new_v_log_scales, *new_v_quats, *new_v_logits, *new_v_sh;
  const unsigned char* fates; const int* offsets; const long* totals;   /* of v3a_densify_classify */
  long U, U_out;
  int K;
  unsigned long long seed; unsigned int step;
  int revised_opacity;
} v3a_densify_apply_args;
int v3a_densify_apply(const v3a_densify_apply_args* a, void* stream);

/* Opacity reset: logit = min(logit, logit(max_opacity)) (fp64 compare, one rounding), m = v = 0, elementwise on [U];
 * max_opacity in (0, 1) (else V3A_ERR_SHAPE). */
int v3a_densify_reset_opacity(float* logits, float* m_logits, float* v_logits, long U, double max_opacity, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scene export packed on the device (csrc/splat_export.hip; the reference's post_opt/exporter.py export_splats: `ply`, `splat`,
 * `ply_compressed`).  DESIGN.md section 7g states the formats.  All five entry points take one struct.
 *
 * Scene: means f32 [U,3], log-scales f32 [U,3], quaternions f32 [U,4] (quats_xyzw != 0: stored x y z w; else w x y z, the files'
 * order), opacity logits f32 [U], harmonics f32 [U,3,K+1] with coefficient 0 the DC term (f_rest_j, j = c K + k, is sh[u][c][1+k]);
 * K >= 0.  ld_*: row strides in ELEMENTS (>= 3, 3, 4, 1, 3 (K+1); a row's own elements are contiguous).  0 <= U < 2^31, K <= 1024
 * (V3A_ERR_SHAPE otherwise).  fp32 throughout, no contraction: a*b + c is two roundings and every division an IEEE division.
 *
 * v3a_splat_export_filter: rows[0 .. *count) = the rows, in ascending order, none of whose values is NaN or Inf and - with
 *   filter_opacity != 0 - whose 1 / (1 + exp(-logit)) > opacity_threshold.  rows int32 [U]; count int64 [1] on the DEVICE (the host
 *   may read it once to size the file).  A flag per row, an integer scan over blocks of 256, one scatter; no atomics.
 *   workspace: v3a_splat_export_filter_workspace_bytes(U, K), 8-byte aligned (too small or misaligned: V3A_ERR_WORKSPACE).
 * v3a_splat_export_sort: order[0 .. n) = rows[0 .. n) by the 30-bit Morton key of their means: per axis
 *   (int32) floor((c - min) / len * 1024) & 0x3ff with min / max over these n rows and a zero length replaced by 1 (the maximum's
 *   1024 becomes 0), bits interleaved with z highest; rocPRIM radix_sort_pairs, stable: equal keys keep ascending row index.
 *   n = the filter's count, as the host read it; order int32 [n].  workspace: v3a_splat_export_sort_workspace_bytes(U, K).
 * v3a_splat_export_pack_compressed (from order): chunk c = sorted splats [256 c, min(256 c + 256, n)).
 *   out_chunks f32 [ceil(n / 256), 18]: min xyz, max xyz of the means; min, max of the log-scales, each clamped to [-20, 20] AFTER
 *     the min / max; min rgb, max rgb of sh0 * 0.28209479 + 0.5.
 *   out_vertices u32 [n,4] (16-byte aligned): position 11-10-11 and scale 11-10-11 of unorm((x - min) / (max - min)); rotation:
 *     q / |q|, largest |component| (lowest index on ties) made positive, its index in bits 31:30, the other three as
 *     unorm10(v * sqrt(2)/2 + 0.5); colour 8-8-8 and unorm8(1 / (1 + exp(-logit))).  unorm_b(v) = clamp(floor(v (2^b - 1) + 0.5), 0,
 *     2^b - 1), and a NaN - the 0 / 0 of a channel whose max == min - gives 0 BY DEFINITION.
 *   out_sh u8 [n, 3K] (4-byte aligned): clamp(trunc((x / 8 + 0.5) * 256), 0, 255) of f_rest_0 .. f_rest_{3K-1}.
 * v3a_splat_export_pack_splat (from order): out_splat [n, 32 bytes] (16-byte aligned): means f32 x 3, exp(log-scale) f32 x 3,
 *   trunc(clamp((rgb, sigmoid) * 255, 0, 255)) u8 x 4, trunc(clamp(q / |q| * 128 + 128, 0, 255)) u8 x 4 (w x y z).
 * v3a_splat_export_pack_ply (from rows, unsorted): out_ply f32 [n, 14 + 3K]: x y z, f_dc_0..2, f_rest_*, logit, log-scales, w x y z.
 * Every output element is written exactly once with plain stores; nothing else is written.  n == 0 is a no-op.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float *means, *log_scales, *quats, *logits, *sh;
  long ld_means, ld_log_scales, ld_quats, ld_logits, ld_sh;
  long U;
  int K, quats_xyzw;
  int filter_opacity; float opacity_threshold;   /* filter only */
  int* rows;        /* filter: out [U]; sort, pack_ply: in [n] */
  long* count;      /* filter: out [1], device */
  long n;           /* sort, pack_*: the survivors, <= U */
  int* order;       /* sort: out [n]; pack_compressed, pack_splat: in */
  float* out_chunks; unsigned int* out_vertices; unsigned char* out_sh;   /* pack_compressed */
  unsigned char* out_splat;                                                /* pack_splat */
  float* out_ply;                                                          /* pack_ply */
  void* workspace; long workspace_bytes;                                   /* filter, sort */
} v3a_splat_export_args;
long v3a_splat_export_filter_workspace_bytes(long U, int K);   /* V3A_ERR_SHAPE for U < 0, U >= 2^31, K < 0 or K > 1024 */
int v3a_splat_export_filter(const v3a_splat_export_args* a, void* stream);
long v3a_splat_export_sort_workspace_bytes(long U, int K);
int v3a_splat_export_sort(const v3a_splat_export_args* a, void* stream);
int v3a_splat_export_pack_compressed(const v3a_splat_export_args* a, void* stream);
int v3a_splat_export_pack_splat(const v3a_splat_export_args* a, void* stream);
int v3a_splat_export_pack_ply(const v3a_splat_export_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scene import decoded on the device (csrc/splat_import.hip): the three files above read back into the trainer's storage.
 * DESIGN.md section 7h states the decoding.  All three entry points take one struct.
 *
 * Outputs (the export kernels' inputs): means f32 [n,3], log-scales f32 [n,3], quaternions f32 [n,4] (quats_xyzw != 0: stored
 * x y z w; else w x y z, the files' order), opacity logits f32 [n], harmonics f32 [n,3,K+1], K = n_rest / 3, coefficient 0 the
 * DC term (f_rest_j, j = c K + k, is sh[u][c][1+k]).  ld_*: row strides in ELEMENTS (>= 3, 3, 4, 1, 3 (K+1)).  Every output
 * element is written exactly once with plain stores; nothing else is written but the workspace.  bad int32 [1] on the DEVICE:
 * the number of rows with a NaN or Inf among their outputs (per-workgroup integer totals in the workspace, summed by one
 * workgroup: no memset, no atomics).
 * Input: `payload`, the file's bytes after the text header, on the device, 4-byte aligned (V3A_ERR_SHAPE otherwise); nothing
 * outside [payload, payload + payload_bytes) is read.  fp32 throughout, no contraction, IEEE divisions; logf / sqrtf are the
 * device library's.
 *
 * v3a_splat_import_ply: rows of P floats; offsets[15] = the columns of x y z, f_dc_0..2, f_rest_0 (f_rest_j at f_rest_0 + j),
 *   opacity, scale_0..2, rot_0..3 (w x y z), all distinct and < P <= 4096; other columns are skipped.  Values are copied;
 *   opacity_linear != 0: logit = logf(o / (1 - o)) of o = the value clamped to [1e-6, 1 - 1e-6] (a NaN stays one).
 *   payload_bytes == 4 n P.
 * v3a_splat_import_compressed: nch == ceil(n / 256) chunks of 18 floats, n vertices of 4 words, n x n_rest bytes;
 *   payload_bytes == 72 nch + 16 n + n n_rest.  Position and log-scale lo + (hi - lo) * (code / top), top = 2047, 1023, 2047;
 *   sh0 = ((lo + (hi - lo) * (code / 255)) - 0.5) / 0.28209479; f_rest = ((byte + 0.5) / 256 - 0.5) * 8; logit =
 *   logf(c / (255 - c)), c = clamp(code, 0.5, 254.5); rotation v = (code / 1023 - 0.5) * sqrt(2), the dropped component
 *   sqrtf(max(0, 1 - sum v^2)) at the index in bits 31:30 (w x y z numbering), the others in ascending order.
 * v3a_splat_import_splat: n records of 32 bytes, n_rest == 0, payload_bytes == 32 n: means copied, logf(scale),
 *   sh0 = ((b + 0.5) / 255 - 0.5) / 0.28209479, logit as above with c = clamp(b + 0.5, 0.5, 254.5), rotation
 *   (b + 0.5 - 128) / 128 (w x y z, not renormalised).
 * Refusals, before any pointer is read: a null struct or (n > 0) a null pointer V3A_ERR_ARG; n < 0 or >= 2^31, n_rest < 0,
 *   n_rest % 3 != 0, n_rest / 3 > 63, an offset >= P or repeated, a row stride too small, a payload size that disagrees
 *   V3A_ERR_SHAPE; workspace smaller than v3a_splat_import_workspace_bytes(n) or not 8-byte aligned V3A_ERR_WORKSPACE.
 *   n == 0 launches nothing (and leaves *bad alone).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  float *means, *log_scales, *quats, *logits, *sh;
  long ld_means, ld_log_scales, ld_quats, ld_logits, ld_sh;
  long n;
  int n_rest, quats_xyzw;
  int* bad;
  const unsigned char* payload; long payload_bytes;
  long nch;                                    /* compressed */
  int opacity_linear, P;                       /* ply */
  int offsets[15];                             /* ply */
  void* workspace; long workspace_bytes;
} v3a_splat_import_args;
long v3a_splat_import_workspace_bytes(long n);   /* V3A_ERR_SHAPE for n < 0 or n >= 2^31 */
int v3a_splat_import_ply(const v3a_splat_import_args* a, void* stream);
int v3a_splat_import_compressed(const v3a_splat_import_args* a, void* stream);
int v3a_splat_import_splat(const v3a_splat_import_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Similarity transforms of a scene (csrc/splat_transform.hip): x' = scale R x + t.  DESIGN.md section 7i states the contract.
 *
 * v3a_splat_transform: input and output scene as above (means, log-scales, quaternions, logits, harmonics f32 [rows,3,K+1]; ld_* /
 *   out_ld_*: row strides in ELEMENTS; quats_xyzw holds for both).  K + 1 must be 1, 4, 9, 16 or 25 (whole bands up to degree 4).
 *   Per row: mean' = (scale R) mean + t in fp32 (fmaf chain, last element first, on the fp32 roundings of scale R and t);
 *   log-scale' = log-scale + (float)log(scale); quat' = q_R (x) quat (Hamilton product; q_R from R in fp64, w >= 0; not
 *   renormalised); logit and band 0 copied; band l = 1..deg of every channel c' = D_l(R) c with Y_l(R d) = D_l(R) Y_l(d) in the
 *   rasteriser's basis (sh_eval), D_l from fp64 rounded to fp32.  out == in with equal strides is allowed (a wave reads its 64
 *   rows whole before it writes); any other overlap is the caller's error.  No atomics, no workspace.
 *   Refusals, before any pointer is read: null struct V3A_ERR_ARG; rows < 0 or >= 2^31, K < 0 V3A_ERR_SHAPE; (rows > 0) a null
 *   input V3A_ERR_ARG, a short input stride V3A_ERR_SHAPE; K + 1 not a band count V3A_ERR_SHAPE; scale not in (0, inf),
 *   |R R^T - I|_max > 1e-6, det R <= 0 or a non-finite t V3A_ERR_ARG; then the outputs as the inputs.  rows == 0 launches nothing.
 * v3a_sh_rotation_matrices: host only.  out f64 [sum_{l=1..deg} (2l+1)^2]: D_1 .. D_deg, each row-major, one after the other;
 *   0 <= deg <= 4 (V3A_ERR_SHAPE), R as above (V3A_ERR_ARG).  D_l(I) = I exactly.
 * v3a_splat_moments: out f64 [10] on the device = n, sum (x - c) [3], sum (x - c)(x - c)^T as xx xy xz yy yz zz, over the n rows
 *   of means (row stride ld_means >= 3 elements), c = centre f64 [3] on the HOST.  fp64; a lane adds its 4 rows of a 1024-row tile
 *   in index order, block_sum<256> of csrc/fixed_sum.h, then one workgroup adds the tiles in the same way: no atomics,
 *   bit-identical run to run and for every ld_means.  workspace: v3a_splat_moments_workspace_bytes(n), 8-byte aligned.  n == 0
 *   writes ten zeros.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  const float *means, *log_scales, *quats, *logits, *sh;
  long ld_means, ld_log_scales, ld_quats, ld_logits, ld_sh;
  float *out_means, *out_log_scales, *out_quats, *out_logits, *out_sh;
  long out_ld_means, out_ld_log_scales, out_ld_quats, out_ld_logits, out_ld_sh;
  long rows;
  int K, quats_xyzw;
  double scale;
  double R[9];      /* row-major */
  double t[3];
} v3a_splat_transform_args;
int v3a_splat_transform(const v3a_splat_transform_args* a, void* stream);
int v3a_sh_rotation_matrices(const double* R, int deg, double* out);
long v3a_splat_moments_workspace_bytes(long n);   /* V3A_ERR_SHAPE for n < 0 or n >= 2^31 */
int v3a_splat_moments(const float* means, long ld_means, long n, const double* centre, double* out, void* workspace,
                      long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
