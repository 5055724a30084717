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
// Two kernels. SET-UP: a lane per triangle transforms, snaps, culls and clips; survivors are appended through a cursor (one atomic per block) to a dense array of 4-byte tile rectangles
// and an array of set-up records (order free: the result is a maximum). TILES: a 256-thread block per 64 x 64 tile keeps the tile as 4096 words of LDS; each wave
// reads 256 rectangles per step and queues those that touch its tile; a hit whose box inside the tile is at most 4 x 4 pixels is rasterised by its lane, larger ones by the whole wave in 8 x 8 stamps;
// LDS atomic max; the block then stores its tile as Depth16 rows. Every tile scans every rectangle: no bins in this version.
#include <algorithm>

#include "../backend.h"
#include "../device/detmath.h"
#include "../device/raster_coverage.h"
#include "../device/sun_shadow_raster.h"

namespace plr {
namespace sunraster {

struct SetupParams {
    const ShadowCascadeInfo* info; const float* transforms; const float* positions; const uint32_t* indices; const Draw* draws;
    ScratchHeader* header; uint32_t* rects; SetupRecord* records;
    uint32_t cascade, drawCount, triangleCount, capacity, transformCount, vertexCount, indexCount;
    int32_t res;
};

using rastercov::edgeAt00; // the coverage rules are shared with "depthPrepassRaster.comp" (device/raster_coverage.h)
using rastercov::topOrLeft;

__global__ __launch_bounds__(256) void sunShadowSetupKernel(SetupParams p) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    // the draw that holds triangle t. The block walks the draws 256 at a time: every thread loads one draw's triangle count, a block-wide prefix sum gives
    // the chunk's first-triangle boundaries in LDS, and each lane bisects them (instead of every lane walking the draws one dependent load after the other)
    __shared__ uint32_t chunkEnd[256];
    __shared__ uint32_t waveTotal[4];
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t lastOfBlock = min(blockIdx.x * 256u + 255u, p.triangleCount - 1u);
    bool found = false;
    uint32_t drawIndex = 0, local = 0, running = 0;
    for (uint32_t chunk = 0; chunk < p.drawCount; chunk += 256u) {
        const uint32_t d = chunk + threadIdx.x;
        uint32_t sum = d < p.drawCount ? p.draws[d].indexCount / 3u : 0u;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)sum, off);
            if ((int)lane >= off) sum += up;
        }
        if (lane == 63u) waveTotal[wave] = sum;
        __syncthreads();
        for (uint32_t w = 0; w < wave; w++) sum += waveTotal[w];
        chunkEnd[threadIdx.x] = running + sum;
        __syncthreads();
        const uint32_t end = chunkEnd[255];
        if (!found && t < p.triangleCount && t < end) {
            uint32_t lo = 0, hi = 255; // the first k with t < chunkEnd[k]
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (t < chunkEnd[mid]) hi = mid; else lo = mid + 1u;
            }
            found = true;
            drawIndex = chunk + lo;
            local = t - (lo ? chunkEnd[lo - 1u] : running);
        }
        running = end;
        __syncthreads();
        if (running > lastOfBlock) break; // (block-uniform) every triangle of the block has its draw
    }
    Draw draw{};
    if (found) draw = p.draws[drawIndex];
    bool reject = false, survivor = false;
    SetupRecord rec{};
    uint32_t rect = 0;
    if (found) {
        const uint64_t at = (uint64_t)draw.firstIndex + (uint64_t)local * 3u;
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
            else {
                const int64_t area = (int64_t)(X[1] - X[0]) * (int64_t)(Y[2] - Y[0]) - (int64_t)(X[2] - X[0]) * (int64_t)(Y[1] - Y[0]);
                if (area > 0) {
                    const int32_t xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
                    const int32_t ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
                    const int32_t ix0 = max(0, (xmin + 127) >> 8), ix1 = min(p.res - 1, (xmax - 128) >> 8);
                    const int32_t iy0 = max(0, (ymin + 127) >> 8), iy1 = min(p.res - 1, (ymax - 128) >> 8);
                    if (ix0 <= ix1 && iy0 <= iy1) {
                        survivor = true;
                        rec.x0 = X[0]; rec.y0 = Y[0]; rec.x1 = X[1]; rec.y1 = Y[1]; rec.x2 = X[2]; rec.y2 = Y[2];
                        rec.boxMin = (uint32_t)ix0 | ((uint32_t)iy0 << 16); rec.boxMax = (uint32_t)ix1 | ((uint32_t)iy1 << 16);
                        rec.e01 = edgeAt00(X[0], Y[0], X[1], Y[1]); rec.e12 = edgeAt00(X[1], Y[1], X[2], Y[2]); rec.e20 = edgeAt00(X[2], Y[2], X[0], Y[0]);
                        rec.area = area;
                        rec.z0 = z[0]; rec.dz1 = z[1] - z[0]; rec.dz2 = z[2] - z[0];
                        rec.topLeft = (topOrLeft(X[1] - X[0], Y[1] - Y[0]) ? 1u : 0u) | (topOrLeft(X[2] - X[1], Y[2] - Y[1]) ? 2u : 0u) | (topOrLeft(X[0] - X[2], Y[0] - Y[2]) ? 4u : 0u);
                        if (xmax - xmin < kNarrowSpan && ymax - ymin < kNarrowSpan) rec.topLeft |= kNarrowFlag;
                        rect = (uint32_t)(ix0 >> 6) | ((uint32_t)(iy0 >> 6) << 8) | ((uint32_t)(ix1 >> 6) << 16) | ((uint32_t)(iy1 >> 6) << 24);
                    }
                }
            }
        }
    }
    // one 64-bit atomic per block hands it a run of slots (the low word is the cursor) and counts its triangles (the high word): a frame's waves adding to
    // the header one by one were most of this kernel's time (measured for 100 k triangles: 1569 waves x 4 atomics on one cache line, 62 us against 18)
    __shared__ uint32_t waveSurvivors[4], waveFound[4], waveRejects[4], blockBase;
    const unsigned long long foundMask = __ballot(found), rejectMask = __ballot(reject), survivorMask = __ballot(survivor);
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

// one fragment of triangle r at pixel (px, py) of the map; tile: the block's 64 x 64 words, (ox, oy) its first pixel
PLR_DI void shadowFragment(const SetupRecord& r, int64_t sx01, int64_t sy01, int64_t sx12, int64_t sy12, int64_t sx20, int64_t sy20, float fa, int px, int py, uint32_t* tile, int ox, int oy) {
    const int64_t e01 = r.e01 + (int64_t)px * sx01 + (int64_t)py * sy01;
    const int64_t e12 = r.e12 + (int64_t)px * sx12 + (int64_t)py * sy12;
    const int64_t e20 = r.e20 + (int64_t)px * sx20 + (int64_t)py * sy20;
    const bool covered = (e01 > 0 || (e01 == 0 && (r.topLeft & 1u))) && (e12 > 0 || (e12 == 0 && (r.topLeft & 2u))) && (e20 > 0 || (e20 == 0 && (r.topLeft & 4u)));
    if (!covered) return;
    const float l1 = (float)e20 / fa, l2 = (float)e01 / fa;
    float zf = (r.z0 + l1 * r.dz1) + l2 * r.dz2;
    zf = fminf(fmaxf(zf, 0.f), 1.f);
    const uint32_t code = (uint32_t)__builtin_rintf(zf * 65535.f);
    atomicMax(&tile[(py - oy) * kTileSize + (px - ox)], code);
}

// The same fragment for a triangle whose snapped vertices span less than 2^15 sub-pixel units (128 pixels) on both axes (kNarrowFlag) - nearly every shadow-map
// triangle. Every pixel of its box lies within that span of every vertex, so the factors of E = dx (Py - Ya) - dy (Px - Xa) are below 2^15, the products below
// 2^30 and E and A below 2^31: the contract's int64 values, computed in 24-bit multiplies, and their conversion to fp32 is one instruction instead of the
// int64 sequence (measured: the tile kernel of a 2048 x 2048 cascade with 49 k drawn triangles 443 -> 367 us).
PLR_DI void shadowFragmentNarrow(const SetupRecord& r, float fa, int px, int py, uint32_t* tile, int ox, int oy) {
    const int32_t Px = px * 256 + 128, Py = py * 256 + 128;
    const int32_t e01 = __mul24(r.x1 - r.x0, Py - r.y0) - __mul24(r.y1 - r.y0, Px - r.x0);
    const int32_t e12 = __mul24(r.x2 - r.x1, Py - r.y1) - __mul24(r.y2 - r.y1, Px - r.x1);
    const int32_t e20 = __mul24(r.x0 - r.x2, Py - r.y2) - __mul24(r.y0 - r.y2, Px - r.x2);
    const bool covered = (e01 > 0 || (e01 == 0 && (r.topLeft & 1u))) && (e12 > 0 || (e12 == 0 && (r.topLeft & 2u))) && (e20 > 0 || (e20 == 0 && (r.topLeft & 4u)));
    if (!covered) return;
    const float l1 = (float)e20 / fa, l2 = (float)e01 / fa;
    float zf = (r.z0 + l1 * r.dz1) + l2 * r.dz2;
    zf = fminf(fmaxf(zf, 0.f), 1.f);
    const uint32_t code = (uint32_t)__builtin_rintf(zf * 65535.f);
    atomicMax(&tile[(py - oy) * kTileSize + (px - ox)], code);
}

// E(i, j) = E(0, 0) + i (-256 dy) + j (256 dx) for the pixel centre (256 i + 128, 256 j + 128)
#define PLR_SUN_RASTER_STEPS(r)                                                                                                                         \
    const int64_t sx01 = -256ll * (int64_t)((r).y1 - (r).y0), sy01 = 256ll * (int64_t)((r).x1 - (r).x0);                                                \
    const int64_t sx12 = -256ll * (int64_t)((r).y2 - (r).y1), sy12 = 256ll * (int64_t)((r).x2 - (r).x1);                                                \
    const int64_t sx20 = -256ll * (int64_t)((r).y0 - (r).y2), sy20 = 256ll * (int64_t)((r).x0 - (r).x2);                                                \
    const float fa = (float)(r).area

// the record lane `src` holds, in every lane (src is wave-uniform)
PLR_DI SetupRecord broadcastRecord(const SetupRecord& r, int src) {
    union Words { SetupRecord rec; int w[sizeof(SetupRecord) / 4]; };
    Words in, out;
    in.rec = r;
    for (size_t k = 0; k < sizeof(SetupRecord) / 4; k++) out.w[k] = __builtin_amdgcn_readlane(in.w[k], src);
    return out.rec;
}

__global__ __launch_bounds__(256) void sunShadowTileKernel(TileParams p) {
    __shared__ uint32_t tile[kTileSize * kTileSize];
    __shared__ uint32_t hitQueue[4][256]; // per wave: the entries of the current step that touch the tile
    const int tx = (int)blockIdx.x, ty = (int)blockIdx.y;
    const int ox = tx * kTileSize, oy = ty * kTileSize;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(kTileSize * kTileSize); i += 256u) tile[i] = 0u;
    __syncthreads();
    const uint32_t n = min(p.header->cursor, p.capacity);
    // the tile's pixels inside the map
    const int tx1 = min(ox + kTileSize - 1, p.res - 1), ty1 = min(oy + kTileSize - 1, p.res - 1);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) p.header->drawn = n;
    // A wave reads 256 rectangles per step (four per lane, one 16-byte load: the array is padded to that), queues the indices of those that touch its tile in
    // LDS and then takes the queue 64 at a time, a record per lane: one memory latency per 256 entries scanned plus one per 64 hits. Measured against 64
    // entries per step with the record fetched behind the rectangle test (tools/shadow_raster_cost.py): the scan went from 1.5 to 0.85 us per thousand
    // entries; the kernel's time in a busy tile is the hits' arithmetic, which this does not change.
    uint32_t* queue = hitQueue[wave];
    const unsigned long long lanesBelow = (1ull << lane) - 1ull;
    auto touches = [&](uint32_t rc) { return (int)(rc & 255u) <= tx && tx <= (int)((rc >> 16) & 255u) && (int)((rc >> 8) & 255u) <= ty && ty <= (int)(rc >> 24); };
    for (uint32_t base = wave * 256u; base < n; base += 1024u) {
        const uint32_t i0 = base + lane * 4u;
        uint4 rc = make_uint4(0u, 0u, 0u, 0u);
        if (i0 < n) rc = *(const uint4*)(p.rects + i0);
        const bool h0 = i0 < n && touches(rc.x), h1 = i0 + 1u < n && touches(rc.y), h2 = i0 + 2u < n && touches(rc.z), h3 = i0 + 3u < n && touches(rc.w);
        const unsigned long long m0 = __ballot(h0), m1 = __ballot(h1), m2 = __ballot(h2), m3 = __ballot(h3);
        const uint32_t c0 = (uint32_t)__popcll(m0), c1 = c0 + (uint32_t)__popcll(m1), c2 = c1 + (uint32_t)__popcll(m2), total = c2 + (uint32_t)__popcll(m3);
        if (total == 0u) continue;
        if (h0) queue[(uint32_t)__popcll(m0 & lanesBelow)] = i0;
        if (h1) queue[c0 + (uint32_t)__popcll(m1 & lanesBelow)] = i0 + 1u;
        if (h2) queue[c1 + (uint32_t)__popcll(m2 & lanesBelow)] = i0 + 2u;
        if (h3) queue[c2 + (uint32_t)__popcll(m3 & lanesBelow)] = i0 + 3u;
        __builtin_amdgcn_wave_barrier(); // (one wave: its LDS operations execute in order)
        for (uint32_t k = 0; k < total; k += 64u) {
            bool hit = k + lane < total;
            int bx0 = 0, by0 = 0, bx1 = -1, by1 = -1;
            SetupRecord r{};
            if (hit) {
                r = p.records[queue[k + lane]];
                bx0 = max((int)(r.boxMin & 0xffffu), ox); by0 = max((int)(r.boxMin >> 16), oy);
                bx1 = min((int)(r.boxMax & 0xffffu), tx1); by1 = min((int)(r.boxMax >> 16), ty1);
                hit = bx0 <= bx1 && by0 <= by1;
            }
            const bool small = hit && bx1 - bx0 < 4 && by1 - by0 < 4;
            if (small) { // the usual shadow-map triangle: its lane walks the <= 16 pixels
                if (r.topLeft & kNarrowFlag) {
                    const float fa = (float)(int32_t)r.area;
                    for (int py = by0; py <= by1; py++)
                        for (int px = bx0; px <= bx1; px++) shadowFragmentNarrow(r, fa, px, py, tile, ox, oy);
                } else {
                    PLR_SUN_RASTER_STEPS(r);
                    for (int py = by0; py <= by1; py++)
                        for (int px = bx0; px <= bx1; px++) shadowFragment(r, sx01, sy01, sx12, sy12, sx20, sy20, fa, px, py, tile, ox, oy);
                }
            }
            unsigned long long large = __ballot(hit && !small);
            while (large) { // the whole wave walks the box in 8 x 8 stamps, with the record broadcast from the lane that holds it
                const int src = __ffsll((long long)large) - 1;
                large &= large - 1ull;
                const SetupRecord u = broadcastRecord(r, src);
                const int lx0 = __builtin_amdgcn_readlane(bx0, src), ly0 = __builtin_amdgcn_readlane(by0, src);
                const int lx1 = __builtin_amdgcn_readlane(bx1, src), ly1 = __builtin_amdgcn_readlane(by1, src);
                if (u.topLeft & kNarrowFlag) { // (wave-uniform)
                    const float fa = (float)(int32_t)u.area;
                    for (int sy = ly0; sy <= ly1; sy += 8)
                        for (int sx = lx0; sx <= lx1; sx += 8) {
                            const int px = sx + (int)(lane & 7u), py = sy + (int)(lane >> 3);
                            if (px <= lx1 && py <= ly1) shadowFragmentNarrow(u, fa, px, py, tile, ox, oy);
                        }
                } else {
                    PLR_SUN_RASTER_STEPS(u);
                    for (int sy = ly0; sy <= ly1; sy += 8)
                        for (int sx = lx0; sx <= lx1; sx += 8) {
                            const int px = sx + (int)(lane & 7u), py = sy + (int)(lane >> 3);
                            if (px <= lx1 && py <= ly1) shadowFragment(u, sx01, sy01, sx12, sy12, sx20, sy20, fa, px, py, tile, ox, oy);
                        }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
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
