// "drawCulling.comp": frustum culling of whole draws on the GPU, in front of the two rasterisers - the step of RenderFrontend::renderScene that tests every
// object's bounding box against the camera frustum (RenderFrontend.cpp:565-569) and against the sun's frustum (:611-646) before it records a draw. Here the test
// runs as a compute pass against exactly the matrices the rasterisers' set-up kernels use, so that it needs no host copy of the GPU-fitted light matrices and a
// culled draw provably has no fragment. One kernel family serves both math modes: every decision is made in fp32 IEEE operations in a fixed order.
// PLR_BUILD_FLAGS: -ffp-contract=off
//
// THE CULL CONTRACT (DESIGN.md "Frustum culling of draws"; tests/draw_culling_reference.py implements it independently and every word of the culled draw arrays
// and of the counters must agree bit for bit). fp32 IEEE, no contraction, every sum left to right as bracketed.
//   inputs: `draws`, the view's draw array (24-byte records {firstIndex, indexCount, vertexOffset, transformIndex, albedo, specular} of the depth prepass for
//     the main view, 16-byte records {firstIndex, indexCount, vertexOffset, transformIndex} of the shadow pass for a shadow view), never modified; `bounds`, six
//     floats {lo.xyz, hi.xyz} per draw: the local box of the draw's mesh over all the mesh's vertices, exact fp32 minima and maxima, computed by the host once
//     when the meshes are set. The main view binds MainPassMatrices[] and uses M = mvp of draws[d].transformIndex; a shadow view of cascade c binds the
//     casters' model matrices and sunShadowInfo. All matrices glm column-major.
//   corners: corner k (0 .. 7) takes hi on axis x, y, z where bit 0, 1, 2 of k is set, and lo otherwise
//   clip components of a corner (x, y, z), as the set-up kernels evaluate them:
//     main view: c_i = ((M[0][i] x + M[1][i] y) + M[2][i] z) + M[3][i] for i = x, y, z, w ("depthPrepassRaster.comp"'s clipComponent)
//     shadow view of cascade c: first M = L_c * T, each element ((a0 b0 + a1 b1) + a2 b2) + a3 b3 (the shadow contract's expression), then c_x and c_y by the
//       same bracketed sum over M's rows; c_w is exactly 1 (the shadow pass does not divide by w)
//   magnitude: a = (max(|lo.x|, |hi.x|), max(|lo.y|, |hi.y|), max(|lo.z|, |hi.z|)), max(p, q) = p > q ? p : q; S_i = ((|M[0][i]| a.x + |M[1][i]| a.y) +
//     |M[2][i]| a.z) + |M[3][i]|; in a shadow view S_w is exactly 1
//   planes, tested in this order: main view: near g = c_z - c_w (reverse Z: inside is w - z >= 0), +x g = c_x - c_w, -x g = (-c_x) - c_w, +y g = c_y - c_w,
//     -y g = (-c_y) - c_w; a shadow view: the last four only. tol = max(2^-100, 2^-16 (S_a + S_w)) with max(p, q) = p > q ? p : q, S_a the magnitude of the
//     plane's own component (z, x, x, y, y). (The floor 2^-100 is the proof's: below it a product may underflow and lose its relative error bound.)
//   decision: a draw is outside a plane when g > tol holds at all eight corners (a NaN compares false). It is culled when it is outside at least one plane; the
//     first such plane in the order is the one counted. Everything else is kept, in particular a draw whose transformIndex is outside its buffer, a draw with
//     a non-finite bound or matrix element and a draw with fewer than three indices (it is tested like any other and counts as visible or culled, with 0
//     triangles). A non-finite bound reaches every S_i, and a non-finite element of a caster's model matrix both rows of L_c * T (0 times an infinity is a
//     NaN), so their comparisons fail by themselves; an mvp element of a component a plane does not read would not stop that plane, so the main view adds one
//     guard: a draw is tested only when ((S_x + S_y) + S_z) + S_w < 2^126 (a NaN compares false), and kept otherwise. Below that limit no clip component, and
//     no difference of two that the clip forms, leaves fp32's range, which the proof relies on
//   absent on purpose: a far plane in the main view (the raster contract's far rule is per fragment, zf > 0, and two fp32 weights can add up to more than 1:
//     a cull there cannot be proved to leave every byte alone) and depth planes in a shadow view (the depth clamp is on: a caster in front of or behind the
//     cascade's range still writes the map). Known false positive: a box outside the frustum across an edge or a corner is outside no single plane and is kept
//   outputs: culledDraws[d] = draws[d] bit for bit, with indexCount = 0 where the draw was culled; per view {visibleDraws, visibleTriangles, culledByPlane[5],
//     pad}, visibleTriangles the sum of indexCount / 3 over the kept draws; a shadow view leaves culledByPlane[0] at 0. The launcher clears the counters on
//     every execution
//   what it guarantees: every image the two rasterisers write from the culled array is byte for byte the image of the same execution with the unculled array
//     (the proof: DESIGN.md). The rasterisers' counters are NOT the unculled execution's: submitted, clipped, drawn and rejects are those of the same pass run
//     on the kept draws alone.
//   deviation from the reference: it tests a world-space box against the frustum of the unjittered camera, far plane included, and for shadows against a frustum
//     fitted to the camera with the near points pushed 10000 units towards the sun (Culling.cpp, RenderFrontend.cpp:614-631); its camera test can drop a draw
//     that the jittered viewProjection still brings onto an edge pixel. This pass tests against the set-up kernels' own matrices.
//
// One kernel, a lane per draw in 256-thread blocks, the view as the grid's second dimension: one execution for the main view, one for all cascades together.
// The counters are reduced by wave ballots and pop-counts (the triangle sum by a wave reduction) and one atomic add per block and counter.
#include <algorithm>

#include "../backend.h"
#include "../device/draw_culling.h"

namespace plr {
namespace drawcull {

struct Params {
    const uint32_t* draws; const float* bounds; const float* transforms; const ShadowCascadeInfo* info;
    ViewStats* stats;
    uint32_t* culled[kMaxViews];
    uint32_t drawCount, transformCount;
};

// the first plane (0 .. 4) the box is outside of, or kPlaneCount. c[k * 4 + i]: component i (x, y, z, w) of corner k; S: the four magnitudes
template <bool kShadow> PLR_DI uint32_t firstOutsidePlane(const float* c, const float* S) {
    for (uint32_t plane = kShadow ? 1u : 0u; plane < kPlaneCount; plane++) {
        const int comp = plane == 0u ? 2 : plane <= 2u ? 0 : 1;
        const bool negate = plane == 2u || plane == 4u;
        const float scaled = kToleranceScale * (S[comp] + S[3]);
        const float tol = kToleranceFloor > scaled ? kToleranceFloor : scaled; // (a NaN stays a NaN)
        bool outside = true;
        for (int k = 0; k < 8; k++) {
            const float a = c[k * 4 + comp];
            const float g = (negate ? -a : a) - c[k * 4 + 3];
            outside = outside && g > tol; // (a NaN compares false)
        }
        if (outside) return plane;
    }
    return kPlaneCount;
}

template <bool kShadow> __global__ __launch_bounds__(256) void drawCullingKernel(Params p) {
    constexpr uint32_t kWords = kShadow ? 4u : 6u; // of a draw record
    const uint32_t d = blockIdx.x * 256u + threadIdx.x, view = blockIdx.y, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool valid = d < p.drawCount;
    uint32_t words[kWords] = {};
    uint32_t plane = kPlaneCount;
    if (valid) {
        for (uint32_t w = 0; w < kWords; w++) words[w] = p.draws[(size_t)d * kWords + w];
        const uint32_t transformIndex = words[3];
        if (transformIndex < p.transformCount) {
            const float* b = p.bounds + (size_t)d * kBoundsFloats;
            const float lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
            float M[16]; // [column * 4 + row]
            if constexpr (kShadow) {
                const float* L = p.info->lightMatrices[view];
                const float* T = p.transforms + (size_t)transformIndex * 16u;
                for (int col = 0; col < 4; col++) {
                    for (int r = 0; r < 2; r++) M[col * 4 + r] = ((L[0 * 4 + r] * T[col * 4 + 0] + L[1 * 4 + r] * T[col * 4 + 1]) + L[2 * 4 + r] * T[col * 4 + 2]) + L[3 * 4 + r] * T[col * 4 + 3];
                    M[col * 4 + 2] = M[col * 4 + 3] = 0.f; // (unused: no depth plane, and w is exactly 1)
                }
            } else {
                const float* mvp = p.transforms + (size_t)transformIndex * 48u + 16u;
                for (int e = 0; e < 16; e++) M[e] = mvp[e];
            }
            float a[3];
            for (int i = 0; i < 3; i++) {
                const float al = fabsf(lo[i]), ah = fabsf(hi[i]);
                a[i] = al > ah ? al : ah;
            }
            float S[4], c[32];
            for (int i = 0; i < 4; i++) S[i] = ((fabsf(M[0 * 4 + i]) * a[0] + fabsf(M[1 * 4 + i]) * a[1]) + fabsf(M[2 * 4 + i]) * a[2]) + fabsf(M[3 * 4 + i]);
            if constexpr (kShadow) S[3] = 1.f;
            for (int k = 0; k < 8; k++) {
                const float x = k & 1 ? hi[0] : lo[0], y = k & 2 ? hi[1] : lo[1], z = k & 4 ? hi[2] : lo[2];
                for (int i = 0; i < 4; i++) c[k * 4 + i] = ((M[0 * 4 + i] * x + M[1 * 4 + i] * y) + M[2 * 4 + i] * z) + M[3 * 4 + i];
                if constexpr (kShadow) c[k * 4 + 3] = 1.f;
            }
            bool testable = true;
            if constexpr (!kShadow) testable = ((S[0] + S[1]) + S[2]) + S[3] < kMagnitudeLimit; // (a NaN compares false)
            if (testable) plane = firstOutsidePlane<kShadow>(c, S);
        }
        const bool culled = plane < kPlaneCount;
        uint32_t* out = p.culled[view] + (size_t)d * kWords;
        for (uint32_t w = 0; w < kWords; w++) out[w] = w == 1u && culled ? 0u : words[w];
    }
    // the counters: ballots and pop-counts per wave, the triangle sum by a wave reduction, one atomic add per block and counter
    const bool kept = valid && plane == kPlaneCount;
    __shared__ uint32_t waveCounts[4][2 + kPlaneCount];
    uint32_t triangles = kept ? words[1] / 3u : 0u;
    for (int off = 32; off > 0; off >>= 1) triangles += (uint32_t)__shfl_down((int)triangles, off);
    const unsigned long long keptMask = __ballot(kept);
    unsigned long long planeMask[kPlaneCount];
    for (uint32_t k = 0; k < kPlaneCount; k++) planeMask[k] = __ballot(valid && plane == k);
    if (lane == 0) {
        waveCounts[wave][0] = (uint32_t)__popcll(keptMask);
        waveCounts[wave][1] = triangles;
        for (uint32_t k = 0; k < kPlaneCount; k++) waveCounts[wave][2 + k] = (uint32_t)__popcll(planeMask[k]);
    }
    __syncthreads();
    if (threadIdx.x < 2u + kPlaneCount) {
        const uint32_t k = threadIdx.x;
        const uint32_t sum = waveCounts[0][k] + waveCounts[1][k] + waveCounts[2][k] + waveCounts[3][k];
        uint32_t* stats = (uint32_t*)(p.stats + view);
        if (sum) atomicAdd(stats + k, sum);
    }
}

static int launchDrawCulling(const PassCtx& c) {
    if (c.push.size() != sizeof(PushConstants)) return c.fail(-1, "drawCulling: push constants {drawCount, viewKind, viewCount} missing (12 bytes)");
    PushConstants pc{};
    std::memcpy(&pc, c.push.data(), sizeof(pc));
    if (c.dispatch[0] != 1u || c.dispatch[1] != 1u || c.dispatch[2] != 1u || c.base[0] != 0u || c.base[1] != 0u)
        return c.fail(-1, "drawCulling: the dispatch is {1, 1, 1} (the launcher derives its grid from the push constants)");
    if (pc.viewKind > kViewShadow) return c.fail(-1, "drawCulling: viewKind is " + std::to_string(pc.viewKind) + ", it must be 0 (the main view) or 1 (shadow views)");
    const bool shadow = pc.viewKind == kViewShadow;
    if (pc.viewCount < 1u || pc.viewCount > (shadow ? kMaxViews : 1u))
        return c.fail(-1, "drawCulling: viewCount is " + std::to_string(pc.viewCount) + ", it must be 1 for the main view and 1 .. 4 for shadow views");
    const size_t drawBytes = shadow ? sizeof(sunraster::Draw) : sizeof(prepass::Draw);
    if (int rc = c.needSbuf(kDrawBinding, (size_t)pc.drawCount * drawBytes, shadow ? "drawCulling draws (16 bytes per draw)" : "drawCulling draws (24 bytes per draw)")) return rc;
    if (int rc = c.needSbuf(kBoundsBinding, (size_t)pc.drawCount * kBoundsFloats * sizeof(float), "drawCulling bounds (6 floats per draw: lo.xyz, hi.xyz)")) return rc;
    if (int rc = c.needSbuf(kTransformBinding, 0, shadow ? "drawCulling transforms (mat4[])" : "drawCulling transforms (MainPassMatrices[]: model, mvp, mvpPrevious)")) return rc;
    if (shadow)
        if (int rc = c.needSbuf(kSunShadowInfoBinding, sizeof(ShadowCascadeInfo), "drawCulling sunShadowInfo")) return rc;
    if (int rc = c.needSbuf(kStatsBinding, statsBytes(pc.viewCount), "drawCulling stats (32 bytes per view)")) return rc;
    for (uint32_t v = 0; v < pc.viewCount; v++)
        if (int rc = c.needSbuf(kCulledDrawBinding + (int)v, (size_t)pc.drawCount * drawBytes, "drawCulling culledDraws (one array of the draws' size per view, bindings 5 ..)")) return rc;
    // outputs are writable and alias neither an input nor each other
    const int inputCount = shadow ? 4 : 3;
    const int outputCount = 1 + (int)pc.viewCount;
    auto output = [&](int k) { return k == 0 ? kStatsBinding : kCulledDrawBinding + k - 1; };
    for (int k = 0; k < outputCount; k++) {
        const int b = output(k);
        if (c.sbuf[b].readOnly) return c.fail(-4, "drawCulling: an output buffer (binding " + std::to_string(b) + ") is bound read-only");
        for (int in = 0; in < inputCount; in++)
            if (c.sbuf[in].ptr == c.sbuf[b].ptr) return c.fail(-4, "drawCulling: the output buffer at binding " + std::to_string(b) + " is also bound as an input (binding " + std::to_string(in) + ")");
        for (int j = 0; j < k; j++)
            if (c.sbuf[output(j)].ptr == c.sbuf[b].ptr)
                return c.fail(-4, "drawCulling: the output buffers at bindings " + std::to_string(output(j)) + " and " + std::to_string(b) + " are the same buffer");
    }
    if (hipMemsetAsync(c.sbuf[kStatsBinding].ptr, 0, statsBytes(pc.viewCount), c.stream) != hipSuccess) return c.fail(-2, "drawCulling: clearing the counters failed");
    if (pc.drawCount == 0u) return 0;
    Params p{};
    p.draws = (const uint32_t*)c.sbuf[kDrawBinding].ptr; p.bounds = (const float*)c.sbuf[kBoundsBinding].ptr; p.transforms = (const float*)c.sbuf[kTransformBinding].ptr;
    p.info = shadow ? (const ShadowCascadeInfo*)c.sbuf[kSunShadowInfoBinding].ptr : nullptr;
    p.stats = (ViewStats*)c.sbuf[kStatsBinding].ptr;
    for (uint32_t v = 0; v < pc.viewCount; v++) p.culled[v] = (uint32_t*)c.sbuf[kCulledDrawBinding + (int)v].ptr;
    p.drawCount = pc.drawCount;
    p.transformCount = (uint32_t)std::min<size_t>(c.sbuf[kTransformBinding].size / (shadow ? 64u : sizeof(prepass::MainPassMatrices)), 0xffffffffu);
    const dim3 grid(divUp(pc.drawCount, 256u), pc.viewCount);
    if (shadow) drawCullingKernel<true><<<grid, 256, 0, c.stream>>>(p);
    else drawCullingKernel<false><<<grid, 256, 0, c.stream>>>(p);
    PLR_CHECK_LAUNCH(c);
    return 0;
}

} // namespace drawcull
static int draw_culling_launch(const PassCtx& c) { return drawcull::launchDrawCulling(c); }
static int draw_culling_launch_fast(const PassCtx& c) { return drawcull::launchDrawCulling(c); }
PLR_REGISTER_SHADER("drawCulling.comp", draw_culling_launch);
PLR_REGISTER_SHADER_FAST("drawCulling.comp", draw_culling_launch_fast);
} // namespace plr
