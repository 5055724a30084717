// What the two compute rasterisers ("sunShadowRaster.comp", "depthPrepassRaster.comp") share on the host side: the limits of the rasterisation contract (DESIGN.md
// "Sun shadow cascades as a compute pass") and the set-up record both tile kernels walk. Each pass's header names them with `using`. Plain C++: no device code here.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace plr {
namespace rastercov {

constexpr int kTileSize = 64;          // pixels per tile edge: one workgroup
constexpr int kMaxResolution = 16384;  // 256 tiles per axis: a tile rectangle is four bytes
constexpr int kSubPixelBits = 8;
constexpr float kGuardBandPixels = 1048576.f; // 2^20
constexpr int32_t kNarrowSpan = 32768;        // a triangle whose snapped vertices span less than this on both axes: its edge functions and its area fit int32
constexpr uint32_t kNarrowFlag = 8u;          // ... flagged in SetupRecord::topLeft

struct alignas(16) SetupRecord {
    int32_t x0, y0, x1, y1, x2, y2;  // snapped vertices, 8 sub-pixel bits
    uint32_t boxMin, boxMax;         // pixel box clipped to the image: x | y << 16, inclusive
    int64_t e01, e12, e20;           // edge functions at the centre of pixel (0, 0)
    int64_t area;                    // A > 0
    float z0, dz1, dz2;              // z0, z1 - z0, z2 - z0
    uint32_t topLeft;                // bit e: edge e (0 -> 1, 1 -> 2, 2 -> 0) is a top or a left edge; kNarrowFlag
};
static_assert(sizeof(SetupRecord) == 80, "SetupRecord layout");

} // namespace rastercov
} // namespace plr
