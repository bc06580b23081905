// Pieces the 3D-Gaussian rasteriser's forward (raster.hip) and backward (raster_bwd.hip) must share word for word: the SH basis
// polynomials and the tile rectangle of a projected Gaussian.  The backward recomputes both and has to land on the same values.
#pragma once
#include "common.h"

namespace gs {

constexpr int TILE = 16;

template <int DEG>
__host__ __device__ __forceinline__ void sh_eval(float x, float y, float z, float* b) {
  b[0] = 0.2820947917738781f;
  if constexpr (DEG >= 1) { b[1] = -0.48860251190292f * y; b[2] = 0.48860251190292f * z; b[3] = -0.48860251190292f * x; }
  if constexpr (DEG >= 2) {
    const float z2 = z * z, t0b = -1.092548430592079f * z, c1 = x * x - y * y, s1 = 2.f * x * y;
    const float p6 = 0.9461746957575601f * z2 - 0.3153915652525201f;
    b[4] = 0.5462742152960395f * s1; b[5] = t0b * y; b[6] = p6; b[7] = t0b * x; b[8] = 0.5462742152960395f * c1;
    if constexpr (DEG >= 3) {
      const float t0c = -2.285228997322329f * z2 + 0.4570457994644658f, t1b = 1.445305721320277f * z;
      const float c2 = x * c1 - y * s1, s2 = x * s1 + y * c1;
      const float p12 = z * (1.865881662950577f * z2 - 1.119528997770346f);
      b[9] = -0.5900435899266435f * s2; b[10] = t1b * s1; b[11] = t0c * y; b[12] = p12; b[13] = t0c * x; b[14] = t1b * c1;
      b[15] = -0.5900435899266435f * c2;
      if constexpr (DEG >= 4) {
        const float t0d = z * (-4.683325804901025f * z2 + 2.007139630671868f), t1c = 3.31161143515146f * z2 - 0.47308734787878f;
        const float t2b = -1.770130769779931f * z, c3 = x * c2 - y * s2, s3 = x * s2 + y * c2;
        b[16] = 0.6258357354491763f * s3; b[17] = t2b * s2; b[18] = t1c * s1; b[19] = t0d * y;
        b[20] = 1.984313483298443f * z * p12 - 1.006230589874905f * p6;
        b[21] = t0d * x; b[22] = t1c * c1; b[23] = t2b * c2; b[24] = 0.6258357354491763f * c3;
      }
    }
  }
}

__host__ __device__ __forceinline__ void tile_bounds(float mx, float my, int radius, int tw, int th, int& x0, int& x1, int& y0, int& y1) {
  const float r = (float)radius / (float)TILE, tx = mx / (float)TILE, ty = my / (float)TILE;
  // (uint32)floor(negative) saturates to 0 on the device gsplat runs on: clamp to [0, grid]
  x0 = (int)fminf(fmaxf(floorf(tx - r), 0.f), (float)tw); x1 = (int)fminf(fmaxf(ceilf(tx + r), 0.f), (float)tw);
  y0 = (int)fminf(fmaxf(floorf(ty - r), 0.f), (float)th); y1 = (int)fminf(fmaxf(ceilf(ty + r), 0.f), (float)th);
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace gs
