// "sunShadowRaster.comp": what the launcher (kernels/sun_shadow_raster.hip) and the frame pipeline (frontend/frame_pipeline.cpp) share - the pass record's
// bindings and the layout of its scratch buffer. Plain C++: no device code here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "raster_record.h"

namespace plr {
namespace sunraster {

// the pass record (DESIGN.md "Sun shadow cascades as a compute pass")
constexpr int kSunShadowInfoBinding = 0, kTransformBinding = 1, kPositionBinding = 2, kIndexBinding = 3, kDrawBinding = 4, kScratchBinding = 5; // storage buffers
constexpr int kMapBinding = 0;                                                                                                                  // storage image, Depth16
constexpr uint32_t kCascadeIndexConstant = 0;
struct PushConstants { uint32_t drawCount, triangleCount; };
struct Draw { uint32_t firstIndex, indexCount, vertexOffset, transformIndex; };

// the contract's limits and the set-up record are the two rasterisers' (device/raster_record.h); this pass keeps its tile as 4096 words of LDS
using rastercov::kGuardBandPixels;
using rastercov::kMaxResolution;
using rastercov::kNarrowFlag;
using rastercov::kNarrowSpan;
using rastercov::kSubPixelBits;
using rastercov::kTileSize;
using rastercov::SetupRecord;

// scratch: header, then one 4-byte tile rectangle per surviving triangle (dense, for the tile kernel's scan), then one set-up record per surviving triangle
struct alignas(8) ScratchHeader {
    uint32_t cursor;    // surviving triangles = entries of the two arrays  } one 64-bit word for the set-up kernel's atomic: the cursor is the low half,
    uint32_t submitted; // triangles the draws hold                          } and it never carries (at most triangleCount < 2^32 survivors)
    uint32_t drawn;     // = cursor, copied by the tile kernel: back faces inside the guard band whose pixel box meets the map
    uint32_t guardBandRejects;
    uint32_t pad[12];
};
static_assert(sizeof(ScratchHeader) == 64, "ScratchHeader layout");

constexpr size_t rectOffset() { return sizeof(ScratchHeader); }
constexpr size_t recordOffset(uint32_t triangleCount) { return sizeof(ScratchHeader) + (((size_t)triangleCount * 4u + 15u) & ~(size_t)15u); }
constexpr size_t scratchBytes(uint32_t triangleCount) { return recordOffset(triangleCount) + (size_t)triangleCount * sizeof(SetupRecord); }

} // namespace sunraster
} // namespace plr
