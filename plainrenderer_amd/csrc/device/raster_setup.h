// What the set-up kernels of the two compute rasterisers share on the device: the draw lookup and the step from three snapped vertices to a set-up record and a
// tile rectangle, by the rasterisation contract (DESIGN.md "Sun shadow cascades as a compute pass").
#pragma once
#include "raster_coverage.h"
#include "raster_record.h"

namespace plr {
namespace rastercov {

struct TriangleSlot { bool found; uint32_t draw, local; }; // triangle `local` of draws[draw]

// The draw that holds triangle t of a 256-thread block's 256 consecutive triangles; called by the whole block. The block walks the draws 256 at a time: every
// thread loads one draw's triangle count, a block-wide prefix sum gives the chunk's first-triangle boundaries in LDS, and each lane bisects them (instead of
// every lane walking the draws one dependent load after the other). A slot at or past drawCount is never loaded from: the guard cannot fire while the boundaries
// are monotone (t < chunkEnd[255] then puts the found slot at or below the last draw with a triangle), so every input whose counts add up keeps its result, and
// a raw record whose draws' triangle counts wrap 32 bits leaves the triangle without a draw instead of reading past `draws`.
template <class DrawT> PLR_DI TriangleSlot drawOfTriangle(const DrawT* draws, uint32_t drawCount, uint32_t triangleCount, uint32_t t) {
    __shared__ uint32_t chunkEnd[256];
    __shared__ uint32_t waveTotal[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t lastOfBlock = min(blockIdx.x * 256u + 255u, triangleCount - 1u);
    TriangleSlot slot{false, 0u, 0u};
    uint32_t running = 0;
    for (uint32_t chunk = 0; chunk < drawCount; chunk += 256u) {
        const uint32_t d = chunk + threadIdx.x;
        uint32_t sum = d < drawCount ? draws[d].indexCount / 3u : 0u;
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
        if (!slot.found && t < triangleCount && t < end) {
            uint32_t lo = 0, hi = 255; // the first k with t < chunkEnd[k]
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if (t < chunkEnd[mid]) hi = mid; else lo = mid + 1u;
            }
            if (chunk + lo < drawCount) slot = TriangleSlot{true, chunk + lo, t - (lo ? chunkEnd[lo - 1u] : running)};
        }
        running = end;
        __syncthreads();
        if (running > lastOfBlock) break; // (block-uniform) every triangle of the block has its draw
    }
    return slot;
}

// A triangle of snapped vertices (X, Y, z) in a width x height image: false where it is not drawn (A <= 0, or no pixel centre in its box); otherwise its record
// and its tile rectangle where `rec` is given
PLR_DI bool setupTriangle(const int32_t X[3], const int32_t Y[3], const float z[3], int32_t width, int32_t height, SetupRecord* rec, uint32_t* rect) {
    const int64_t area = (int64_t)(X[1] - X[0]) * (int64_t)(Y[2] - Y[0]) - (int64_t)(X[2] - X[0]) * (int64_t)(Y[1] - Y[0]);
    if (area <= 0) return false;
    const int32_t xmin = min(X[0], min(X[1], X[2])), xmax = max(X[0], max(X[1], X[2]));
    const int32_t ymin = min(Y[0], min(Y[1], Y[2])), ymax = max(Y[0], max(Y[1], Y[2]));
    const int32_t ix0 = max(0, (xmin + 127) >> 8), ix1 = min(width - 1, (xmax - 128) >> 8);
    const int32_t iy0 = max(0, (ymin + 127) >> 8), iy1 = min(height - 1, (ymax - 128) >> 8);
    if (ix0 > ix1 || iy0 > iy1) return false;
    if (rec) {
        SetupRecord& r = *rec;
        r.x0 = X[0]; r.y0 = Y[0]; r.x1 = X[1]; r.y1 = Y[1]; r.x2 = X[2]; r.y2 = Y[2];
        r.boxMin = (uint32_t)ix0 | ((uint32_t)iy0 << 16); r.boxMax = (uint32_t)ix1 | ((uint32_t)iy1 << 16);
        r.e01 = edgeAt00(X[0], Y[0], X[1], Y[1]); r.e12 = edgeAt00(X[1], Y[1], X[2], Y[2]); r.e20 = edgeAt00(X[2], Y[2], X[0], Y[0]);
        r.area = area;
        r.z0 = z[0]; r.dz1 = z[1] - z[0]; r.dz2 = z[2] - z[0];
        r.topLeft = (topOrLeft(X[1] - X[0], Y[1] - Y[0]) ? 1u : 0u) | (topOrLeft(X[2] - X[1], Y[2] - Y[1]) ? 2u : 0u) | (topOrLeft(X[0] - X[2], Y[0] - Y[2]) ? 4u : 0u);
        if (xmax - xmin < kNarrowSpan && ymax - ymin < kNarrowSpan) r.topLeft |= kNarrowFlag;
        *rect = (uint32_t)(ix0 >> 6) | ((uint32_t)(iy0 >> 6) << 8) | ((uint32_t)(ix1 >> 6) << 16) | ((uint32_t)(iy1 >> 6) << 24);
    }
    return true;
}

} // namespace rastercov
} // namespace plr
