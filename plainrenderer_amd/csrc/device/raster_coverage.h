// What the two compute rasterisers ("sunShadowRaster.comp", "depthPrepassRaster.comp") share on the device: the integer coverage rules of the rasterisation
// contract (DESIGN.md "Sun shadow cascades as a compute pass"). Vertices are snapped to 8 sub-pixel bits, the triangle has A > 0, the pixel centre of (i, j) is
// (256 i + 128, 256 j + 128), and for an edge a -> b: E = (Xb - Xa)(Py - Ya) - (Yb - Ya)(Px - Xa) in int64.
#pragma once
#include <stdint.h>

#include "detmath.h"

namespace plr {
namespace rastercov {

// a top (dy == 0 && dx > 0) or a left (dy < 0) edge, d = b - a, in a y-down frame: a pixel centre ON such an edge is covered
PLR_DI bool topOrLeft(int32_t dx, int32_t dy) { return (dy == 0 && dx > 0) || dy < 0; }
// E of the edge a -> b at the centre of pixel (0, 0)
PLR_DI int64_t edgeAt00(int32_t xa, int32_t ya, int32_t xb, int32_t yb) { return (int64_t)(xb - xa) * (int64_t)(128 - ya) - (int64_t)(yb - ya) * (int64_t)(128 - xa); }
// covered: every E > 0, or E == 0 on a top or left edge (bit e of topLeft: edge e of 0 -> 1, 1 -> 2, 2 -> 0)
template <class I> PLR_DI bool covered(I e01, I e12, I e20, uint32_t topLeft) {
    return (e01 > 0 || (e01 == 0 && (topLeft & 1u))) && (e12 > 0 || (e12 == 0 && (topLeft & 2u))) && (e20 > 0 || (e20 == 0 && (topLeft & 4u)));
}

} // namespace rastercov
} // namespace plr
