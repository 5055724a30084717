// What the tile kernels of the two compute rasterisers share on the device: a wave's scan of the rectangle list for its 64 x 64 tile and its walk of the hits,
// fragment by fragment, by the rasterisation contract (DESIGN.md "Sun shadow cascades as a compute pass"). What becomes of a fragment is the pass's.
#pragma once
#include "raster_coverage.h"
#include "raster_record.h"

namespace plr {
namespace rastercov {

// E(i, j) = E(0, 0) + i (-256 dy) + j (256 dx) for the pixel centre (256 i + 128, 256 j + 128)
struct EdgeSteps {
    int64_t sx01, sy01, sx12, sy12, sx20, sy20;
    float fa;
    PLR_DI explicit EdgeSteps(const SetupRecord& r)
        : sx01(-256ll * (int64_t)(r.y1 - r.y0)), sy01(256ll * (int64_t)(r.x1 - r.x0)), sx12(-256ll * (int64_t)(r.y2 - r.y1)), sy12(256ll * (int64_t)(r.x2 - r.x1)),
          sx20(-256ll * (int64_t)(r.y0 - r.y2)), sy20(256ll * (int64_t)(r.x0 - r.x2)), fa((float)r.area) {}
};

// coverage and depth of triangle r at pixel (px, py): false where the pixel centre is not covered, else the contract's zf and, where `weights` is given, the
// fp32 weights l1, l2 it was formed from (a pass that interpolates more than depth; a null `weights` is a compile-time one and leaves no trace)
PLR_DI bool fragmentDepth(const SetupRecord& r, const EdgeSteps& s, int px, int py, float* zf, float* weights = nullptr) {
    const int64_t e01 = r.e01 + (int64_t)px * s.sx01 + (int64_t)py * s.sy01;
    const int64_t e12 = r.e12 + (int64_t)px * s.sx12 + (int64_t)py * s.sy12;
    const int64_t e20 = r.e20 + (int64_t)px * s.sx20 + (int64_t)py * s.sy20;
    if (!covered(e01, e12, e20, r.topLeft)) return false;
    const float l1 = (float)e20 / s.fa, l2 = (float)e01 / s.fa;
    *zf = (r.z0 + l1 * r.dz1) + l2 * r.dz2;
    if (weights) { weights[0] = l1; weights[1] = l2; }
    return true;
}

// The same for a triangle whose snapped vertices span less than 2^15 sub-pixel units (128 pixels) on both axes (kNarrowFlag) - nearly every triangle. Every
// pixel of its box lies within that span of every vertex, so the factors of E = dx (Py - Ya) - dy (Px - Xa) are below 2^15, the products below 2^30 and E and A
// below 2^31: the contract's int64 values, computed in 24-bit multiplies, and their conversion to fp32 is one instruction instead of the int64 sequence
// (measured: the shadow tile kernel of a 2048 x 2048 cascade with 49 k drawn triangles 443 -> 367 us). fa: (float)(int32_t)r.area, which is (float)r.area.
PLR_DI bool fragmentDepthNarrow(const SetupRecord& r, float fa, int px, int py, float* zf, float* weights = nullptr) {
    const int32_t Px = px * 256 + 128, Py = py * 256 + 128;
    const int32_t e01 = __mul24(r.x1 - r.x0, Py - r.y0) - __mul24(r.y1 - r.y0, Px - r.x0);
    const int32_t e12 = __mul24(r.x2 - r.x1, Py - r.y1) - __mul24(r.y2 - r.y1, Px - r.x1);
    const int32_t e20 = __mul24(r.x0 - r.x2, Py - r.y2) - __mul24(r.y0 - r.y2, Px - r.x2);
    if (!covered(e01, e12, e20, r.topLeft)) return false;
    const float l1 = (float)e20 / fa, l2 = (float)e01 / fa;
    *zf = (r.z0 + l1 * r.dz1) + l2 * r.dz2;
    if (weights) { weights[0] = l1; weights[1] = l2; }
    return true;
}

// what lane `src` holds, in every lane (src is wave-uniform)
template <class T> PLR_DI T broadcastLane(const T& v, int src) {
    static_assert(sizeof(T) % 4 == 0, "moved word by word");
    union Words { T v; int w[sizeof(T) / 4]; };
    Words in, out;
    in.v = v;
    for (size_t k = 0; k < sizeof(T) / 4; k++) out.w[k] = __builtin_amdgcn_readlane(in.w[k], src);
    return out.v;
}

// The pixels x0 .. x1, y0 .. y1 of triangle r, kStride x kStride at a time with this lane at (offx, offy) of each: fragment(px, py, depthAt) for every pixel of
// the lane, inside the box or not; depthAt(&zf) is false outside the box and where the pixel centre is not covered, else it gives the depth, and
// depthAt(&zf, weights) the depth's two fp32 weights l1, l2 with it. kStride 1: a lane walks a box of its own; 8: the wave walks one box in 8 x 8 stamps, and
// all lanes arrive at every call together.
template <int kStride, class F> PLR_DI void walkBox(const SetupRecord& r, int x0, int y0, int x1, int y1, int offx, int offy, F&& fragment) {
    auto walk = [&](auto&& depthOf) {
        for (int sy = y0; sy <= y1; sy += kStride)
            for (int sx = x0; sx <= x1; sx += kStride) {
                const int px = sx + offx, py = sy + offy;
                fragment(px, py, [&](float* zf, float* weights = nullptr) { return px <= x1 && py <= y1 && depthOf(px, py, zf, weights); });
            }
    };
    if (r.topLeft & kNarrowFlag) {
        const float fa = (float)(int32_t)r.area;
        walk([&](int px, int py, float* zf, float* weights) { return fragmentDepthNarrow(r, fa, px, py, zf, weights); });
    } else {
        const EdgeSteps steps(r);
        walk([&](int px, int py, float* zf, float* weights) { return fragmentDepth(r, steps, px, py, zf, weights); });
    }
}

struct TileWindow { int tx, ty, ox, oy, x1, y1; }; // the tile, its first pixel and its last pixel inside the image

// The hooks of a pass whose fragments need nothing but themselves. A pass derives from this and adds
//   static const SetupRecord& setup(const Record&)                                     the set-up record inside its record
//   void fragment(const Record&, int slot, int px, int py, depthAt)                    one pixel of a walked box (walkBox); slot: the lane that fetched the record
struct PlainWalk {
    // per step of 64 hits, by the whole wave, before the walk: this lane's record (if `hit`) and its box inside the tile
    template <class Record> PLR_DI void beginStep(const Record&, bool hit, bool small, int bx0, int by0, int bx1, int by1) {}
    PLR_DI bool lanePath() const { return true; }           // does this lane's small record take the lane path?
    PLR_DI bool beginStamps(int src) { return true; }       // (wave-uniform) does the record of lane `src` take the stamp path?
    PLR_DI void endStep() {}                                // by the whole wave, before the next step's records replace these
};

// A wave's part of a tile: it reads 256 rectangles per step (four per lane, one 16-byte load: the array is padded to that), queues the indices of those that
// touch its tile in LDS (`queue`: 256 words of the wave's own) and then takes the queue 64 at a time, a record per lane: one memory latency per 256 entries
// scanned plus one per 64 hits (measured against 64 entries per step with the record fetched behind the rectangle test, tools/shadow_raster_cost.py: the scan
// went from 1.5 to 0.85 us per thousand entries). A hit whose box inside the tile is at most 4 x 4 pixels is walked by its lane, larger ones by the whole wave
// in 8 x 8 stamps, with the record broadcast from the lane that holds it.
template <class Record, class Pass>
PLR_DI void rasteriseTile(const uint32_t* rects, const Record* records, uint32_t n, const TileWindow& w, uint32_t* queue, Pass& pass) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long lanesBelow = (1ull << lane) - 1ull;
    auto touches = [&](uint32_t rc) { return (int)(rc & 255u) <= w.tx && w.tx <= (int)((rc >> 16) & 255u) && (int)((rc >> 8) & 255u) <= w.ty && w.ty <= (int)(rc >> 24); };
    for (uint32_t base = wave * 256u; base < n; base += 1024u) {
        const uint32_t i0 = base + lane * 4u;
        uint4 rc = make_uint4(0u, 0u, 0u, 0u);
        if (i0 < n) rc = *(const uint4*)(rects + i0);
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
            Record rr{};
            if (hit) {
                rr = records[queue[k + lane]];
                const SetupRecord& r = Pass::setup(rr);
                bx0 = max((int)(r.boxMin & 0xffffu), w.ox); by0 = max((int)(r.boxMin >> 16), w.oy);
                bx1 = min((int)(r.boxMax & 0xffffu), w.x1); by1 = min((int)(r.boxMax >> 16), w.y1);
                hit = bx0 <= bx1 && by0 <= by1;
            }
            const bool small = hit && bx1 - bx0 < 4 && by1 - by0 < 4;
            pass.beginStep(rr, hit, small, bx0, by0, bx1, by1);
            if (small && pass.lanePath())
                walkBox<1>(Pass::setup(rr), bx0, by0, bx1, by1, 0, 0, [&](int px, int py, auto&& depthAt) { pass.fragment(rr, (int)lane, px, py, depthAt); });
            unsigned long long large = __ballot(hit && !small);
            while (large) {
                const int src = __ffsll((long long)large) - 1;
                large &= large - 1ull;
                if (!pass.beginStamps(src)) continue;
                const Record u = broadcastLane(rr, src);
                const int lx0 = __builtin_amdgcn_readlane(bx0, src), ly0 = __builtin_amdgcn_readlane(by0, src);
                const int lx1 = __builtin_amdgcn_readlane(bx1, src), ly1 = __builtin_amdgcn_readlane(by1, src);
                walkBox<8>(Pass::setup(u), lx0, ly0, lx1, ly1, (int)(lane & 7u), (int)(lane >> 3), [&](int px, int py, auto&& depthAt) { pass.fragment(u, src, px, py, depthAt); });
            }
            pass.endStep();
        }
        __builtin_amdgcn_wave_barrier();
    }
}

} // namespace rastercov
} // namespace plr
