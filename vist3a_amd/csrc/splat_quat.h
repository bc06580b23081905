// The two activations of a raw Gaussian as the post-optimisation kernels form them, each defined once.  quat_R: the rotation of a
// raw quaternion behind v3a_splat_activate (and its backward) in post_opt.hip, in float, and behind v3a_mcmc_noise in mcmc.hip and
// the split children of densify.hip, in double.  sigmoid64: the opacity of a logit behind mcmc.hip, densify.hip and splat_reg.hip.
// Included by those four files only.
#pragma once

// rotation of a quaternion (i, j, k, r), normalised the way the adapter normalises it (gaussian_adapter_kernel, elementwise.hip).
// T = float is the arithmetic of v3a_splat_activate; T = double is the same expression evaluated in fp64 on exactly converted
// inputs, the float constant 1e-8f included.
template <typename T>
__device__ __forceinline__ void quat_R(const T* qin, T* R) {
  T q[4], n2 = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) { q[e] = qin[e]; n2 += q[e] * q[e]; }
  const T inv = T(1) / (sqrt(n2) + T(1e-8f));
#pragma unroll
  for (int e = 0; e < 4; ++e) q[e] *= inv;
  const T i = q[0], j = q[1], k = q[2], r = q[3];
  const T two_s = T(2) / (i * i + j * j + k * k + r * r);
  R[0] = 1 - two_s * (j * j + k * k); R[1] = two_s * (i * j - k * r);     R[2] = two_s * (i * k + j * r);
  R[3] = two_s * (i * j + k * r);     R[4] = 1 - two_s * (i * i + k * k); R[5] = two_s * (j * k - i * r);
  R[6] = two_s * (i * k - j * r);     R[7] = two_s * (j * k + i * r);     R[8] = 1 - two_s * (i * i + j * j);
}

// opacity of a logit in fp64 on the exactly converted input.  No product feeds a sum, so contraction cannot change it: the same
// bits above or below a file's `#pragma clang fp contract(off)`.
__device__ __forceinline__ double sigmoid64(float x) { return 1.0 / (1.0 + exp(-(double)x)); }
