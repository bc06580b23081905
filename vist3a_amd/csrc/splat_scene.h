// A scene as the strategy and file kernels handle it, stated once: the order of its five tensors, the floats in a row of each, the
// strided view of splat_export.hip, splat_import.hip and splat_transform.hip with its validation, and the contiguous parameter /
// moment sets of mcmc.hip and densify.hip.  Included by those five files only, after common.h.
#pragma once

enum { SPLAT_MEANS, SPLAT_LS, SPLAT_QUATS, SPLAT_LOGITS, SPLAT_SH, SPLAT_FIELDS };   // the order in every struct of vist3a_hip.h
enum { SPLAT_PARAMS, SPLAT_M, SPLAT_V, SPLAT_GROUPS };                               // the values, Adam's first and second moments
// the five pointers of *a whose names begin with `pre`, in that order: SPLAT_SET(a, ), SPLAT_SET(a, m_), SPLAT_SET(a, new_v_)
#define SPLAT_SET(a, pre) {(a)->pre##means, (a)->pre##log_scales, (a)->pre##quats, (a)->pre##logits, (a)->pre##sh}

constexpr float SH_C0 = 0.28209479177387814f;
__device__ __forceinline__ bool finite32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// floats in a row of `field`; n_sh is the harmonics' share: 3 K, or 3 (K + 1) where the DC term is stored with the rest
__host__ __device__ constexpr int splat_width(int field, int n_sh) {
  return field == SPLAT_QUATS ? 4 : field == SPLAT_LOGITS ? 1 : field == SPLAT_SH ? n_sh : 3;
}

// Rows ld[f] elements apart, a row's own elements contiguous; harmonics [rows,3,K+1].  T = const float reads a scene, float writes one.
template <class T>
struct SplatView {
  T* p[SPLAT_FIELDS]; long ld[SPLAT_FIELDS]; long rows; int K, xyzw;
  __device__ T* means(long r) const { return p[SPLAT_MEANS] + r * ld[SPLAT_MEANS]; }
  __device__ T* ls(long r) const { return p[SPLAT_LS] + r * ld[SPLAT_LS]; }
  __device__ T* quats(long r) const { return p[SPLAT_QUATS] + r * ld[SPLAT_QUATS]; }
  __device__ T& logit(long r) const { return p[SPLAT_LOGITS][r * ld[SPLAT_LOGITS]]; }
  __device__ T* sh(long r) const { return p[SPLAT_SH] + r * ld[SPLAT_SH]; }
  __device__ int quat_slot(int e) const { return xyzw ? (e + 3) & 3 : e; }   // where component e of the files' order (w x y z) is stored
};

// The view of v3a_splat_export_args, v3a_splat_import_args or either half of v3a_splat_transform_args (the same field names): V3A_OK - with v left alone when there are no
// rows - or the error code, after which v means nothing.  No pointer is read through.
template <class Args, class T>
int splat_view_of(const Args* a, long rows, int K, SplatView<T>& v) {
  if (!a) return V3A_ERR_ARG;
  if (bad_count(rows) || K < 0) return V3A_ERR_SHAPE;
  if (rows == 0) return V3A_OK;
  v = {SPLAT_SET(a, ), {a->ld_means, a->ld_log_scales, a->ld_quats, a->ld_logits, a->ld_sh}, rows, K, a->quats_xyzw != 0};
  for (int f = 0; f < SPLAT_FIELDS; ++f)
    if (!v.p[f]) return V3A_ERR_ARG;
  for (int f = 0; f < SPLAT_FIELDS; ++f)
    if (v.ld[f] < splat_width(f, 3 * (K + 1))) return V3A_ERR_SHAPE;
  return V3A_OK;
}

// One group (SPLAT_PARAMS, SPLAT_M or SPLAT_V) of contiguous tensors [rows, splat_width(f, 3 K)]
template <class T>
struct SplatSet {
  T* t[SPLAT_FIELDS];
  __host__ __device__ T* operator[](int f) const { return t[f]; }
};
template <class T>
bool splat_sets_have_null(const SplatSet<T>* g) {   // g[SPLAT_GROUPS]
  for (int i = 0; i < SPLAT_GROUPS * SPLAT_FIELDS; ++i)
    if (!g[i / SPLAT_FIELDS][i % SPLAT_FIELDS]) return true;
  return false;
}
