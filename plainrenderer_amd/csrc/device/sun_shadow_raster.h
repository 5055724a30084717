// "sunShadowRaster.comp": what the launcher (kernels/sun_shadow_raster.hip) and the frame pipeline (frontend/frame_pipeline.cpp) share - the pass record's
// bindings and the layout of its scratch buffer. Plain C++: no device code here.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace plr {
namespace sunraster {

// the pass record (DESIGN.md "Sun shadow cascades as a compute pass")
constexpr int kSunShadowInfoBinding = 0, kTransformBinding = 1, kPositionBinding = 2, kIndexBinding = 3, kDrawBinding = 4, kScratchBinding = 5; // storage buffers
constexpr int kMapBinding = 0;                                                                                                                  // storage image, Depth16
constexpr uint32_t kCascadeIndexConstant = 0;
struct PushConstants { uint32_t drawCount, triangleCount; };
struct Draw { uint32_t firstIndex, indexCount, vertexOffset, transformIndex; };

constexpr int kTileSize = 64;          // pixels per tile edge: one workgroup, 4096 words of LDS
constexpr int kMaxResolution = 16384;  // 256 tiles per axis: a tile rectangle is four bytes
constexpr int kSubPixelBits = 8;
constexpr float kGuardBandPixels = 1048576.f; // 2^20
constexpr int32_t kNarrowSpan = 32768;        // a triangle whose snapped vertices span less than this on both axes: its edge functions and its area fit int32
constexpr uint32_t kNarrowFlag = 8u;          // ... flagged in SetupRecord::topLeft

// scratch: header, then one 4-byte tile rectangle per surviving triangle (dense, for the tile kernel's scan), then one set-up record per surviving triangle
struct alignas(8) ScratchHeader {
    uint32_t cursor;    // surviving triangles = entries of the two arrays  } one 64-bit word for the set-up kernel's atomic: the cursor is the low half,
    uint32_t submitted; // triangles the draws hold                          } and it never carries (at most triangleCount < 2^32 survivors)
    uint32_t drawn;     // = cursor, copied by the tile kernel: back faces inside the guard band whose pixel box meets the map
    uint32_t guardBandRejects;
    uint32_t pad[12];
};
static_assert(sizeof(ScratchHeader) == 64, "ScratchHeader layout");

struct alignas(16) SetupRecord {
    int32_t x0, y0, x1, y1, x2, y2;  // snapped vertices, 8 sub-pixel bits
    uint32_t boxMin, boxMax;         // pixel box clipped to the map: x | y << 16, inclusive
    int64_t e01, e12, e20;           // edge functions at the centre of pixel (0, 0)
    int64_t area;                    // A > 0
    float z0, dz1, dz2;              // z0, z1 - z0, z2 - z0
    uint32_t topLeft;                // bit e: edge e (0 -> 1, 1 -> 2, 2 -> 0) is a top or a left edge; kNarrowFlag
};
static_assert(sizeof(SetupRecord) == 80, "SetupRecord layout");

constexpr size_t rectOffset() { return sizeof(ScratchHeader); }
constexpr size_t recordOffset(uint32_t triangleCount) { return sizeof(ScratchHeader) + (((size_t)triangleCount * 4u + 15u) & ~(size_t)15u); }
constexpr size_t scratchBytes(uint32_t triangleCount) { return recordOffset(triangleCount) + (size_t)triangleCount * sizeof(SetupRecord); }

} // namespace sunraster
} // namespace plr
