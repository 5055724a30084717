// "sunShadowRaster.comp": the sun shadow cascades as a compute pass - RenderFrontend::renderSunShadowCascades (RenderFrontend.cpp:354, 760-774; pass description
// :1565-1590; sunShadow.vert / sunShadow.frag) for opaque casters: depth only, orthographic, one Depth16 target per execution. One kernel family serves both math
// modes: every decision is an integer one and the float part is a dozen IEEE operations per fragment.
// PLR_BUILD_FLAGS: -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt
//
// THE RASTERISATION CONTRACT (DESIGN.md "Sun shadow cascades as a compute pass"; tests/shadow_raster_reference.py implements it independently and every texel
// and counter must agree bit for bit). fp32 IEEE, no contraction. Cascade c, L = sunShadowInfo.lightMatrices[c], a draw with model matrix T, both column-major:
//   M = L * T first (GLSL's A * B * v is (A * B) * v, sunShadow.vert:29), each element a0 b0 + a1 b1 + a2 b2 + a3 b3 summed left to right
//   clip = M * (p, 1), each component m[0][i] x + m[1][i] y + m[2][i] z + m[3][i] summed left to right; w is not divided by: T is affine (the host boundary
//     refuses anything else) and L orthographic (lightMatrix.comp:57-138)
//   viewport 0 .. res on both axes, no Y flip, depth 0 .. 1 (VulkanCommandRecording.cpp:44-48): xf = (clip.x * 0.5 + 0.5) * res, yf likewise, z = clip.z
//   X = rint(xf * 256), Y = rint(yf * 256), round to nearest even, int32: eight sub-pixel bits
//   guard band: a triangle with a non-finite xf, yf or z, or |xf| or |yf| >= 2^20 pixels, is not drawn and counted as a reject (no clipping). Inside the band
//     every product below fits int64.
//   outside a buffer: a triangle counts as submitted and as a reject, and draws nothing, when its three index slots are not all inside `indices`, when a
//     vertex (index + vertexOffset, in 64 bits) is not inside `positions`, or when its draw's transformIndex is not inside `transforms`. A draw submits
//     indexCount / 3 triangles (rounded down), whatever becomes of them.
//   A = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0); Vulkan's area is -A / 2 and the front face counter-clockwise (VulkanPipeline.cpp:61), so A < 0 faces front;
//     the pass culls FRONT faces (RenderFrontend.cpp:1576): only A > 0 is drawn
//   pixel box: columns (Xmin + 127) >> 8 .. (Xmax - 128) >> 8 (the pixel centres 256 i + 128 inside [Xmin, Xmax]) clipped to 0 .. res - 1, rows likewise; a
//     triangle with an empty box is dropped, every other one counts as drawn
//   edges 0 -> 1, 1 -> 2, 2 -> 0; for a -> b and the pixel centre P = (256 i + 128, 256 j + 128): E = (Xb - Xa)(Py - Ya) - (Yb - Ya)(Px - Xa), int64
//   a pixel is covered when every E > 0, or E == 0 on a top (dy == 0 && dx > 0) or left (dy < 0) edge, d = b - a: the top-left rule in a y-down frame
//   l1 = float(E_20) / float(A), l2 = float(E_01) / float(A) (int64 -> fp32 to nearest even, IEEE divide); zf = (z0 + l1 (z1 - z0)) + l2 (z2 - z0)
//   depth clamp on (:1578): zf to [0, 1] as fmin(fmax(zf, 0), 1) with IEEE maxNum / minNum semantics (of a NaN and a number, the number): a NaN zf - finite
//     vertex depths whose difference overflows, times a zero weight - stores code 0, +inf stores 65535; code = rint(zf * 65535) as uint16
//   cleared to 0, depth test GreaterEqual (RenderPass.cpp:105, :1574): a texel is the MAXIMUM code of its fragments, 0 without any. Every texel of the map is
//     written by every execution: the clear is part of the pass.
//   sunShadow.frag's alpha test is left out - casters are opaque: its anisotropic repeat sampler is implementation-defined and material textures are no input here.
//
// Two kernels. SET-UP: a lane per triangle finds its draw, transforms, snaps, culls and boxes; survivors are appended through a cursor (one atomic per block) to a dense
// array of 4-byte tile rectangles and an array of set-up records (order free: the result is a maximum). TILES: a 256-thread block per 64 x 64 tile keeps the tile as
// 4096 words of LDS; each wave scans the rectangles and walks those that touch its tile; LDS atomic max; the block then stores its tile as Depth16 rows. Every tile
// scans every rectangle: no bins in this version. The draw lookup and the record are device/raster_setup.h's, the scan, the walk and a fragment's coverage and
// depth device/raster_tile_walk.h's, both shared with "depthPrepassRaster.comp"; this file holds the transform, the block's append, what becomes of a fragment
// (clamp, encode, maximum), the tile's store and the launcher.
#include <algorithm>

#include "../backend.h"
#include "../device/detmath.h"
#include "../device/raster_setup.h"
#include "../device/raster_tile_walk.h"
#include "../device/sun_shadow_raster.h"

namespace plr {
namespace sunraster {

struct SetupParams {
    const ShadowCascadeInfo* info; const float* transforms; const float* positions; const uint32_t* indices; const Draw* draws;
    ScratchHeader* header; uint32_t* rects; SetupRecord* records;
    uint32_t cascade, drawCount, triangleCount, capacity, transformCount, vertexCount, indexCount;
    int32_t res;
};

__global__ __launch_bounds__(256) void sunShadowSetupKernel(SetupParams p) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const rastercov::TriangleSlot found = rastercov::drawOfTriangle(p.draws, p.drawCount, p.triangleCount, t);
    Draw draw{};
    if (found.found) draw = p.draws[found.draw];
    bool reject = false, survivor = false;
    SetupRecord rec{};
    uint32_t rect = 0;
    if (found.found) {
        const uint64_t at = (uint64_t)draw.firstIndex + (uint64_t)found.local * 3u;
        bool inBuffers = at + 3u <= (uint64_t)p.indexCount && draw.transformIndex < p.transformCount;
        uint64_t v[3] = {0, 0, 0};
        if (inBuffers)
            for (int k = 0; k < 3; k++) {
                v[k] = (uint64_t)p.indices[at + k] + (uint64_t)draw.vertexOffset;
                inBuffers = inBuffers && v[k] < (uint64_t)p.vertexCount;
            }
        if (!inBuffers) reject = true;
        else {
            const float* L = p.info->lightMatrices[p.cascade];
            const float* T = p.transforms + (size_t)draw.transformIndex * 16u;
            float M[12]; // rows 0 .. 2 of the four columns: M[c * 3 + r]
            for (int c = 0; c < 4; c++)
                for (int r = 0; r < 3; r++) M[c * 3 + r] = ((L[0 * 4 + r] * T[c * 4 + 0] + L[1 * 4 + r] * T[c * 4 + 1]) + L[2 * 4 + r] * T[c * 4 + 2]) + L[3 * 4 + r] * T[c * 4 + 3];
            const float resf = (float)p.res;
            int32_t X[3], Y[3];
            float z[3];
            bool inside = true;
            for (int k = 0; k < 3; k++) {
                const float* q = p.positions + v[k] * 3u;
                const float x = q[0], y = q[1], zz = q[2];
                const float cx = ((M[0] * x + M[3] * y) + M[6] * zz) + M[9];
                const float cy = ((M[1] * x + M[4] * y) + M[7] * zz) + M[10];
                const float cz = ((M[2] * x + M[5] * y) + M[8] * zz) + M[11];
                const float xf = (cx * 0.5f + 0.5f) * resf, yf = (cy * 0.5f + 0.5f) * resf;
                // (a NaN or an infinity fails the comparisons)
                const bool ok = fabsf(xf) < kGuardBandPixels && fabsf(yf) < kGuardBandPixels && fabsf(cz) < __builtin_inff();
                inside = inside && ok;
                X[k] = ok ? (int32_t)__builtin_rintf(xf * 256.f) : 0;
                Y[k] = ok ? (int32_t)__builtin_rintf(yf * 256.f) : 0;
                z[k] = cz;
            }
            if (!inside) reject = true;
            else survivor = rastercov::setupTriangle(X, Y, z, p.res, p.res, &rec, &rect);
        }
    }
    // one 64-bit atomic per block hands it a run of slots (the low word is the cursor) and counts its triangles (the high word): a frame's waves adding to
    // the header one by one were most of this kernel's time (measured for 100 k triangles: 1569 waves x 4 atomics on one cache line, 62 us against 18)
    // (the prepass appends 0 .. 6 records per lane through a prefix sum of counts; this is one survivor per lane by ballot, and neither form serves the other)
    __shared__ uint32_t waveSurvivors[4], waveFound[4], waveRejects[4], blockBase;
    const unsigned long long foundMask = __ballot(found.found), rejectMask = __ballot(reject), survivorMask = __ballot(survivor);
    if (lane == 0) { waveSurvivors[wave] = (uint32_t)__popcll(survivorMask); waveFound[wave] = (uint32_t)__popcll(foundMask); waveRejects[wave] = (uint32_t)__popcll(rejectMask); }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t survivors = waveSurvivors[0] + waveSurvivors[1] + waveSurvivors[2] + waveSurvivors[3];
        const uint32_t foundHere = waveFound[0] + waveFound[1] + waveFound[2] + waveFound[3], rejects = waveRejects[0] + waveRejects[1] + waveRejects[2] + waveRejects[3];
        const unsigned long long old = atomicAdd((unsigned long long*)&p.header->cursor, (unsigned long long)survivors | ((unsigned long long)foundHere << 32));
        blockBase = (uint32_t)old;
        if (rejects) atomicAdd(&p.header->guardBandRejects, rejects);
    }
    __syncthreads();
    uint32_t base = blockBase;
    for (uint32_t w = 0; w < wave; w++) base += waveSurvivors[w];
    if (survivor) {
        const uint32_t slot = base + (uint32_t)__popcll(survivorMask & ((1ull << lane) - 1ull));
        if (slot < p.capacity) { // (always: the cursor counts at most triangleCount survivors and the launcher sized the arrays for that many)
            p.rects[slot] = rect;
            p.records[slot] = rec;
        }
    }
}

struct TileParams {
    ScratchHeader* header; const uint32_t* rects; const SetupRecord* records;
    uint16_t* map;
    uint32_t capacity;
    int32_t res;
};

// what becomes of a fragment: depth clamp, Depth16 code, maximum. tile: the block's 64 x 64 words
struct ShadowWalk : rastercov::PlainWalk {
    uint32_t* tile;
    int ox, oy;
    static PLR_DI const SetupRecord& setup(const SetupRecord& r) { return r; }
    template <class D> PLR_DI void fragment(const SetupRecord&, int, int px, int py, D&& depthAt) {
        float zf;
        if (!depthAt(&zf)) return;
        zf = fminf(fmaxf(zf, 0.f), 1.f);
        const uint32_t code = (uint32_t)__builtin_rintf(zf * 65535.f);
        atomicMax(&tile[(py - oy) * kTileSize + (px - ox)], code);
    }
};

__global__ __launch_bounds__(256) void sunShadowTileKernel(TileParams p) {
    __shared__ uint32_t tile[kTileSize * kTileSize];
    __shared__ uint32_t hitQueue[4][256]; // per wave: the entries of the current step that touch the tile
    const int tx = (int)blockIdx.x, ty = (int)blockIdx.y;
    const int ox = tx * kTileSize, oy = ty * kTileSize;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(kTileSize * kTileSize); i += 256u) tile[i] = 0u;
    __syncthreads();
    const uint32_t n = min(p.header->cursor, p.capacity);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.header->drawn = n;
    // the kernel's time in a busy tile is the hits' arithmetic
    const rastercov::TileWindow window{tx, ty, ox, oy, min(ox + kTileSize - 1, p.res - 1), min(oy + kTileSize - 1, p.res - 1)};
    ShadowWalk walk{{}, tile, ox, oy};
    rastercov::rasteriseTile(p.rects, p.records, n, window, hitQueue[wave], walk);
    __syncthreads();
    // the tile as Depth16 rows: eight texels per 16-byte store where the eight lie inside the map and the address allows, texel by texel at ragged edges
    const bool rowsAligned = (p.res & 7) == 0;
    for (uint32_t c = threadIdx.x; c < (uint32_t)(kTileSize * kTileSize / 8); c += 256u) {
        const int row = (int)(c >> 3), col = (int)(c & 7u) * 8;
        const int y = oy + row, x = ox + col;
        if (y >= p.res || x >= p.res) continue;
        const uint32_t* src = tile + row * kTileSize + col;
        uint16_t* dst = p.map + (size_t)y * (size_t)p.res + (size_t)x;
        if (rowsAligned && x + 8 <= p.res) {
            uint4 v;
            v.x = src[0] | (src[1] << 16); v.y = src[2] | (src[3] << 16); v.z = src[4] | (src[5] << 16); v.w = src[6] | (src[7] << 16);
            *(uint4*)dst = v;
        } else {
            for (int k = 0; k < 8 && x + k < p.res; k++) dst[k] = (uint16_t)src[k];
        }
    }
}

static int launchSunShadowRaster(const PassCtx& c) {
    const uint32_t cascade = c.specUint(kCascadeIndexConstant, 0u);
    if (cascade >= 4u) return c.fail(-1, "sunShadowRaster: cascadeIndex (specialisation constant 0) is " + std::to_string(cascade) + ", a sunShadowInfo block holds 4 light matrices");
    if (c.push.size() < sizeof(PushConstants)) return c.fail(-1, "sunShadowRaster: push constants {drawCount, triangleCount} missing");
    PushConstants pc;
    std::memcpy(&pc, c.push.data(), sizeof(pc));
    if (c.dispatch[0] != 1u || c.dispatch[1] != 1u || c.dispatch[2] != 1u || c.base[0] != 0u || c.base[1] != 0u)
        return c.fail(-1, "sunShadowRaster: the dispatch is {1, 1, 1} (the launcher derives its grids from the push constants and the map)");
    if (int rc = c.needSbuf(kSunShadowInfoBinding, sizeof(ShadowCascadeInfo), "sunShadowRaster sunShadowInfo")) return rc;
    if (int rc = c.needSbuf(kTransformBinding, 0, "sunShadowRaster transforms (mat4[])")) return rc;
    if (int rc = c.needSbuf(kPositionBinding, 0, "sunShadowRaster positions (3 floats per vertex)")) return rc;
    if (int rc = c.needSbuf(kIndexBinding, 0, "sunShadowRaster indices (uint32 triangle list)")) return rc;
    if (int rc = c.needSbuf(kDrawBinding, (size_t)pc.drawCount * sizeof(Draw), "sunShadowRaster draws {firstIndex, indexCount, vertexOffset, transformIndex}")) return rc;
    if (int rc = c.needSbuf(kScratchBinding, scratchBytes(pc.triangleCount), "sunShadowRaster scratch (64 + 16 ceil(triangleCount / 4) + 80 triangleCount bytes)")) return rc;
    if (c.sbuf[kScratchBinding].readOnly) return c.fail(-4, "sunShadowRaster: the scratch buffer (binding 5) is bound read-only");
    if (int rc = c.needStorage(kMapBinding, F_D16, "sunShadowRaster shadow map")) return rc;
    const ImgView map = c.storage[kMapBinding];
    if (map.w != map.h || map.w < 1 || map.w > kMaxResolution || map.d > 1)
        return c.fail(-4, "sunShadowRaster: the shadow map is " + std::to_string(map.w) + " x " + std::to_string(map.h) + ", it must be square, 2D and at most 16384 texels wide");
    if ((pc.drawCount == 0u) != (pc.triangleCount == 0u)) return c.fail(-1, "sunShadowRaster: drawCount and triangleCount must both be zero or both be non-zero");
    for (int b : {kTransformBinding, kPositionBinding, kIndexBinding, kDrawBinding, kSunShadowInfoBinding})
        if (c.sbuf[b].ptr == c.sbuf[kScratchBinding].ptr) return c.fail(-4, "sunShadowRaster: the scratch buffer is also bound as an input");

    uint8_t* scratch = (uint8_t*)c.sbuf[kScratchBinding].ptr;
    if (hipMemsetAsync(scratch, 0, sizeof(ScratchHeader), c.stream) != hipSuccess) return c.fail(-2, "sunShadowRaster: clearing the scratch header failed");
    if (pc.triangleCount) {
        SetupParams s{};
        s.info = (const ShadowCascadeInfo*)c.sbuf[kSunShadowInfoBinding].ptr; s.transforms = (const float*)c.sbuf[kTransformBinding].ptr;
        s.positions = (const float*)c.sbuf[kPositionBinding].ptr; s.indices = (const uint32_t*)c.sbuf[kIndexBinding].ptr; s.draws = (const Draw*)c.sbuf[kDrawBinding].ptr;
        s.header = (ScratchHeader*)scratch; s.rects = (uint32_t*)(scratch + rectOffset()); s.records = (SetupRecord*)(scratch + recordOffset(pc.triangleCount));
        s.cascade = cascade; s.drawCount = pc.drawCount; s.triangleCount = pc.triangleCount; s.capacity = pc.triangleCount;
        s.transformCount = (uint32_t)std::min<size_t>(c.sbuf[kTransformBinding].size / 64u, 0xffffffffu);
        s.vertexCount = (uint32_t)std::min<size_t>(c.sbuf[kPositionBinding].size / 12u, 0xffffffffu);
        s.indexCount = (uint32_t)std::min<size_t>(c.sbuf[kIndexBinding].size / 4u, 0xffffffffu);
        s.res = map.w;
        sunShadowSetupKernel<<<divUp(pc.triangleCount, 256u), 256, 0, c.stream>>>(s);
        PLR_CHECK_LAUNCH(c);
        c.splitTiming("set-up");
    }
    TileParams t{};
    t.header = (ScratchHeader*)scratch; t.rects = (const uint32_t*)(scratch + rectOffset()); t.records = (const SetupRecord*)(scratch + recordOffset(pc.triangleCount));
    t.map = (uint16_t*)map.ptr; t.capacity = pc.triangleCount; t.res = map.w;
    const unsigned tiles = divUp((unsigned)map.w, (unsigned)kTileSize);
    sunShadowTileKernel<<<dim3(tiles, tiles), 256, 0, c.stream>>>(t);
    PLR_CHECK_LAUNCH(c);
    return 0;
}

} // namespace sunraster
static int sun_shadow_raster_launch(const PassCtx& c) { return sunraster::launchSunShadowRaster(c); }
static int sun_shadow_raster_launch_fast(const PassCtx& c) { return sunraster::launchSunShadowRaster(c); }
PLR_REGISTER_SHADER("sunShadowRaster.comp", sun_shadow_raster_launch);
PLR_REGISTER_SHADER_FAST("sunShadowRaster.comp", sun_shadow_raster_launch_fast);
} // namespace plr
