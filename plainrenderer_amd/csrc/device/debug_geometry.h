// "debugGeometry.comp": what the launcher (kernels/debug_geometry.hip) and the frame pipeline (frontend/frame_pipeline.cpp) share - the pass record's bindings,
// its push record and the layout of its counters and scratch. Plain C++: no device code here.
//
// The pass draws one-pixel lines into the frame's colour and depth images, depth-tested against what the frame has written: the twelve edges of the world box of
// every scene draw, the twelve edges of every SDF instance's padded world box, and the caller's own segments (DESIGN.md "Debug geometry as a compute pass").
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "depth_prepass_raster.h"

namespace plr {
namespace debuggeo {

// the pass record. A source whose count is 0 binds nothing
constexpr int kDrawBinding = 0;      // storage buffers: prepass::Draw[] (24 bytes per draw), read-only; with drawsCulled the culled copy of "drawCulling.comp"
constexpr int kBoundsBinding = 1;    // 6 floats per draw {lo.xyz, hi.xyz}: the local box of the draw's mesh ("drawCulling.comp"'s bounds), read-only
constexpr int kTransformBinding = 2; // MainPassMatrices[] (the model matrix is used), read-only
constexpr int kSdfBoxBinding = 3;    // BoundingBox[] (32 bytes: min.xyz, pad, max.xyz, pad), read-only
constexpr int kLineBinding = 4;      // 9 floats per line {a.xyz, b.xyz, rgb}, read-only
constexpr int kStatsBinding = 5;     // Stats, cleared by the launcher on every execution
constexpr int kColorBinding = 0;     // storage images: the frame's colour (R11G11B10) ...
constexpr int kDepthBinding = 1;     // ... and depth (Depth32), of one size
struct PushConstants { uint32_t drawCount, sdfBoxCount, lineCount, drawsCulled; }; // drawsCulled 1: a draw with indexCount 0 submits nothing
static_assert(sizeof(PushConstants) == 16, "the pass record");

struct Stats {
    uint32_t submitted;     // segments the sources hold: 12 per box that submits, 1 per line
    uint32_t clipped;       // segments with an end replaced on a clip plane, whatever became of them afterwards
    uint32_t rejected;      // segments dropped by a plane or by an end's validity rule
    uint32_t drawn;         // segments with at least one major pixel index inside the image
    uint32_t fragments;     // fragments that passed the depth test
    uint32_t pixelsWritten; // pixels with a winner
    uint32_t pad[2];
};
static_assert(sizeof(Stats) == 32, "Stats layout");

constexpr uint32_t kEdgesPerBox = 12;
constexpr uint32_t kChunkSteps = 64;             // major steps per work item: a wave
constexpr uint32_t kMaxLines = 1u << 20;         // what plrf_set_debug_lines accepts
constexpr uint64_t kMaxSegments = 0x7fffffffull; // s + 1 fits the low word of a key with bit 31 free for the record's major flag
constexpr size_t kBoundsFloats = 6, kLineFloats = 9;
constexpr float kDrawBoxColor[3] = {1.f, 0.f, 0.f}, kSdfBoxColor[3] = {0.f, 1.f, 0.f}; // debug.frag's red; green

// one surviving segment, ends ordered along the major axis
struct alignas(16) Record {
    int32_t u0, v0, u1, v1; // snapped ends, 8 sub-pixel bits: major, minor
    float z0, z1;
    uint32_t color;         // the R11G11B10 word
    uint32_t sAndMajor;     // s | (y-major ? 1 << 31 : 0)
};
static_assert(sizeof(Record) == 32, "Record layout");
struct WorkItem { uint32_t record, firstStep; }; // major pixel indices firstStep .. firstStep + 63, as far as the segment reaches

// the pass's persistent scratch: the 64-bit keys of width x height pixels first (all 0 between executions), then the header, the records and the work list
struct alignas(16) ScratchHeader { uint32_t records, items, pad[14]; };
static_assert(sizeof(ScratchHeader) == 64, "ScratchHeader layout");
constexpr size_t keyBytes(uint32_t width, uint32_t height) { return (size_t)width * height * 8u; }
constexpr uint64_t segmentCount(uint32_t draws, uint32_t sdfBoxes, uint32_t lines) { return ((uint64_t)draws + sdfBoxes) * kEdgesPerBox + lines; }
constexpr uint32_t chunksPerSegment(uint32_t width, uint32_t height) { return ((width > height ? width : height) + kChunkSteps - 1u) / kChunkSteps; } // upper bound

} // namespace debuggeo
} // namespace plr
