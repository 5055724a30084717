// "drawCulling.comp": what the launcher (kernels/draw_culling.hip) and the frame pipeline (frontend/frame_pipeline.cpp) share - the pass record's bindings, its
// push record and the layout of its outputs. Plain C++: no device code here.
//
// The pass writes, per view, a copy of the view's draw array in which a draw that lies outside one plane of the view's clip volume has indexCount = 0, and a
// block of counters. The two rasterisers consume the copy at their draw binding unchanged (rastercov::drawOfTriangle skips a draw without triangles). Under
// culling the rasterisers' own counters (submitted, clipped, drawn, rejects) are those of the same pass run on the kept draws alone, not those of the unculled
// execution; every image byte is the unculled execution's (DESIGN.md "Frustum culling of draws").
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "depth_prepass_raster.h"
#include "sun_shadow_raster.h"

namespace plr {
namespace drawcull {

// the pass record. One execution serves one kind of view: the main view (the depth prepass's draws against mvp of MainPassMatrices), or all shadow cascades
// together (the casters against lightMatrices[c] * model, the cascade as the grid's second dimension)
constexpr int kDrawBinding = 0;          // the view's draw array, read-only: prepass::Draw (24 bytes) for the main view, sunraster::Draw (16 bytes) for shadow views
constexpr int kBoundsBinding = 1;        // 6 floats per draw {lo.xyz, hi.xyz}: the local box of the draw's mesh, read-only
constexpr int kTransformBinding = 2;     // main view: MainPassMatrices[]; shadow views: the casters' model matrices (mat4[]), read-only
constexpr int kSunShadowInfoBinding = 3; // shadow views only: ShadowCascadeInfo, read-only
constexpr int kStatsBinding = 4;         // kStatsWords uint32 per view, view after view; cleared by the launcher on every execution
constexpr int kCulledDrawBinding = 5;    // 5 + v: the culled copy of view v of the execution (main: v = 0; shadow: v = cascade, up to 4)
constexpr uint32_t kMaxViews = 4;
constexpr uint32_t kViewMain = 0, kViewShadow = 1;
struct PushConstants { uint32_t drawCount, viewKind, viewCount; }; // viewCount: 1 for the main view, the cascade count (1 .. 4) for shadow views
static_assert(sizeof(PushConstants) == 12, "the pass record");

// planes in test order: near, +x, -x, +y, -y (a shadow view tests the last four only)
constexpr uint32_t kPlaneCount = 5;
// the counters of one view
struct ViewStats {
    uint32_t visibleDraws;
    uint32_t visibleTriangles; // sum of indexCount / 3 over the kept draws
    uint32_t culledByPlane[kPlaneCount]; // the first plane, in test order, that a culled draw is outside of
    uint32_t pad;
};
constexpr uint32_t kStatsWords = 8;
static_assert(sizeof(ViewStats) == kStatsWords * 4u, "ViewStats layout");
constexpr size_t statsBytes(uint32_t viewCount) { return (size_t)viewCount * sizeof(ViewStats); }
constexpr size_t kBoundsFloats = 6;
constexpr float kToleranceScale = 1.52587890625e-05f; // 2^-16: tol = max(2^-100, 2^-16 (S_a + S_w))
constexpr float kToleranceFloor = 7.88860905221011805412e-31f; // 2^-100
constexpr float kMagnitudeLimit = 8.50705917302346158658e+37f; // 2^126: the main view tests a draw only while the sum of its four magnitudes is below it

} // namespace drawcull
} // namespace plr
