// The counter-based random numbers of the post-optimisation strategies: Philox4x32-10, its 53-bit uniforms and Box-Muller normals.
// One definition behind mcmc.hip and densify.hip (and v3a_mcmc_philox / v3a_mcmc_uniform, the host's known-answer entry points).
// Include it inside the file's anonymous namespace, AFTER its `#pragma clang fp contract(off)`: nothing here may be contracted.
// Random numbers only: the opacity both files draw against (sigmoid64) is in splat_quat.h.
#pragma once

struct Rand4 { uint32_t x[4]; };

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3")
__host__ __device__ inline Rand4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Rand4 r;
  r.x[0] = c0; r.x[1] = c1; r.x[2] = c2; r.x[3] = c3;
  return r;
}

// 53 bits of two words -> a double in [0, 1); every step is exact
__host__ __device__ inline double uniform53(uint32_t x0, uint32_t x1) {
  return ((double)(x0 >> 5) * 67108864.0 + (double)(x1 >> 6)) * (1.0 / 9007199254740992.0);
}

struct Key { uint32_t k0, k1, stream, step; };

// the draw of (slot, stream) at `step`: counter (slot, 0, stream, step), key = the seed, low word first
__device__ __forceinline__ Rand4 draw(const Key& k, uint32_t slot, uint32_t stream) {
  return philox4x32_10(slot, 0u, stream, k.step, k.k0, k.k1);
}

// Box-Muller in fp64: u1 from words (0, 1), u2 from (2, 3).  cos(2 pi u2) and sin(2 pi u2) as cospi / sinpi of 2 u2 (2 u2 is exact):
// the argument reduction is exact and needs no large-argument path.
__device__ __forceinline__ void normal_pair(const Rand4& r, double& z0, double& z1) {
  const double u1 = uniform53(r.x[0], r.x[1]), u2 = uniform53(r.x[2], r.x[3]);
  const double rad = sqrt(-2.0 * log(1.0 - u1));
  z0 = rad * cospi(2.0 * u2);
  z1 = rad * sinpi(2.0 * u2);
}

inline Key make_key(unsigned long long seed, unsigned int stream, unsigned int step) {
  Key k;
  k.k0 = (uint32_t)(seed & 0xffffffffull);
  k.k1 = (uint32_t)(seed >> 32);
  k.stream = stream;
  k.step = step;
  return k;
}
