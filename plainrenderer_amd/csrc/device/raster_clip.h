// Clip space to the sub-pixel grid, as the rasterisation contract of "depthPrepassRaster.comp" words it: the device code that pass and "debugGeometry.comp" share,
// so that a line end and a triangle vertex with the same clip coordinates land on the same sub-pixel. Only included by files built with -ffp-contract=off and
// -fhip-fp32-correctly-rounded-divide-sqrt: every expression here is fp32 IEEE in the order written.
#pragma once
#include "depth_prepass_raster.h"
#include "detmath.h"

namespace plr {
namespace prepass {

// clip = M * (p, 1) for a glm column-major matrix, component i
PLR_DI float clipComponent(const float* M, int i, float x, float y, float z) { return ((M[0 * 4 + i] * x + M[1 * 4 + i] * y) + M[2 * 4 + i] * z) + M[3 * 4 + i]; }

// the five clip planes in their order: near (reverse Z), then the four sides of the guard volume. A vertex is inside when the distance is >= 0
constexpr int kClipPlanes = 5;
PLR_DI float planeDistance(int plane, float x, float y, float z, float w) {
    switch (plane) {
    case 0: return w - z;
    case 1: return kGuardNdc * w - x;
    case 2: return kGuardNdc * w + x;
    case 3: return kGuardNdc * w - y;
    default: return kGuardNdc * w + y;
    }
}

// a clipped vertex to the sub-pixel grid: ndc = (x / w, y / w), z = clip.z / w, xf = (ndc.x * 0.5 + 0.5) * width, no Y flip; usable when w > 0, |xf| and |yf|
// are below 2^20 and z is finite (a NaN fails). X = rint(xf * 256), Y likewise; 0 where the vertex is not usable
PLR_DI bool projectAndSnap(float x, float y, float z, float w, float widthF, float heightF, int32_t* X, int32_t* Y, float* zOut) {
    const float nx = x / w, ny = y / w, nz = z / w;
    const float xf = (nx * 0.5f + 0.5f) * widthF, yf = (ny * 0.5f + 0.5f) * heightF;
    const bool ok = w > 0.f && fabsf(xf) < rastercov::kGuardBandPixels && fabsf(yf) < rastercov::kGuardBandPixels && fabsf(nz) < __builtin_inff();
    *X = ok ? (int32_t)__builtin_rintf(xf * 256.f) : 0;
    *Y = ok ? (int32_t)__builtin_rintf(yf * 256.f) : 0;
    *zOut = nz;
    return ok;
}

} // namespace prepass
} // namespace plr
