// "debugGeometry.comp": the debug geometry pass as a compute pass - RenderFrontend::renderDebugGeometry (RenderFrontend.cpp:375-378, 947-956; pass description
// :1599-1617; debug.vert / debug.frag; the box mesh :1518-1543; the per-frame box matrices :656-681): one-pixel, depth-tested lines into the frame's colour
// (R11G11B10) and depth (Depth32) images, right behind the deferred shade. Three sources feed it: the world box of every scene draw (the reference's "Render
// bounding boxes"), the padded world box of every SDF instance, and the caller's own segments. One kernel family serves both math modes: every decision is an
// integer or an IEEE one.
// PLR_BUILD_FLAGS: -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt
//
// THE LINE CONTRACT (DESIGN.md "Debug geometry as a compute pass"; tests/debug_lines_reference.py implements it independently and every word of the two images and
// of the counters must agree bit for bit). fp32 IEEE, no contraction, correctly rounded divide, except where fp64 (IEEE, no contraction) is named.
//   1. segments. Segment s = 0, 1, ... in submission order: draw boxes, SDF boxes, the caller's lines. A box has 12 edges: s = 12 * box + edge, box counting the
//      draws first and then the SDF instances; line l has s = 12 (drawCount + sdfBoxCount) + l. A box that submits nothing leaves its twelve numbers unused.
//      draw box d: {lo, hi} = bounds[d] (the local box packDrawBounds keeps), model = transforms[draws[d].transformIndex].model, glm column-major. Corner k takes
//        hi on the axes whose bit of k is set. World component r of a corner (x, y, z) is ((m[0][r] x + m[1][r] y) + m[2][r] z) + m[3][r]. The world box is the
//        minimum and maximum over the corners k = 0 .. 7 in that order: lo = c_0, then lo = c_k < lo ? c_k : lo; hi = c_0, then hi = c_k > hi ? c_k : hi (a NaN
//        corner 0 stays, a later one is skipped). It is the axis-aligned world box the reference draws (obj.bbWorld), not the oriented one. A draw whose
//        transformIndex is outside `transforms` submits nothing; with drawsCulled = 1 - the draw array is the culled copy of "drawCulling.comp" - a draw with
//        indexCount = 0 submits nothing either (only visible boxes are drawn, :665).
//      SDF box i: {min, max} of entry i of the bound BoundingBox array (32 bytes each).
//      edges: for axis a = 0, 1, 2, for ascending corner k with bit a clear: (corner k, corner k | 1 << a) of the world box; edge = 4 a + its place in that order.
//      colours: draw boxes (1, 0, 0) (debug.frag), SDF boxes (0, 1, 0), a line its own rgb; packed once per segment with packR11G11B10Exact in both math modes;
//        not pre-exposed (as in the reference).
//   2. clip and snap. clip = g_viewProjection * (p, 1) per end - the jittered matrix of the `global` block (:670) -, each component by clipComponent. For each of
//      the prepass's five planes, in its order, with its planeDistance d: an end is outside when !(d >= 0) (d < 0 or a NaN). Both ends outside: the segment is
//      dropped and counts as rejected. One end outside: it is replaced by I + t (O - I), t = d_I / (d_I - d_O), per component (x, y, z, w), and the segment counts
//      as clipped (once, and whatever becomes of it later). Then each end needs w > 0, a finite z = clip.z / w and |xf|, |yf| < 2^20 with
//      xf = (x / w * 0.5 + 0.5) * width, no Y flip (projectAndSnap, shared with the prepass); otherwise the segment counts as rejected. X = rint(xf * 256), Y likewise.
//   3. coverage, in integers. dX = X1 - X0, dY = Y1 - Y0. x-major when |dX| >= |dY|, else y-major; U is the major coordinate, V the minor, EU and EV the image
//      extents along them. The ends are exchanged, with their z, when U0 > U1. dU = U1 - U0; dU = 0 covers nothing. Major pixel indices i from
//      max(0, (U0 + 127) >> 8) to min(EU - 1, (U1 - 129) >> 8) (arithmetic shifts): the pixel centres c = 256 i + 128 with U0 <= c < U1. The minor index is
//      j = floor((V0 dU + (c - U0) dV) / (256 dU)) in int64, a floor division. (i, j) is a fragment when 0 <= j < EV. A segment with at least one major index in
//      range counts as drawn.
//   4. depth, fp64: t = double(c - U0) / double(dU), zf = float(double(z0) + t * (double(z1) - double(z0))). A fragment is kept when zf > 0 and zf >= depth[pixel]
//      (a NaN fails both): GreaterEqual against the image as the pass found it. Kept fragments count as fragments.
//   5. visibility. A pixel's winner is the maximum of (bits(zf) << 32) | s over its kept fragments; it stores its colour word and zf; pixels_written counts
//      winners. No other pixel of either image is written or changed. Depth write is on, as in the reference: a line pixel over the sky has a depth above 0.
//   counters: {submitted, clipped, rejected, drawn, fragments, pixels_written, 0, 0}; the launcher clears them on every execution.
//
// Three launches. SET-UP: a lane per segment number generates the segment from its source, clips, projects, snaps and orients it; a survivor - a segment that is
// drawn - gets a 32-byte record, and its major steps are split into chunks of 64 that are appended as {record, first step} items to a work list; records, items
// and every counter take one aggregated atomic add per wave. RASTER A and B: a persistent grid walks the work list, a wave per item and a lane per major step. A
// evaluates coverage and depth and does a 64-bit atomic max on the key scratch (one word per pixel, the key with s + 1 in the low word, 0 = empty); B re-evaluates
// its fragment, and where the scratch word equals its own key it stores colour and depth and puts the word back to 0. A loser's key equals neither the winner's
// nor 0, so the reset needs no ordering within the launch, the scratch is all 0 between executions, and no launch touches a pixel without a fragment: the
// cost follows the fragments. The order of the work list is free: the result is a maximum.
#include <algorithm>

#include "../backend.h"
#include "../device/debug_geometry.h"
#include "../device/raster_clip.h"

namespace plr {
namespace debuggeo {

struct SetupParams {
    const prepass::Draw* draws; const float* bounds; const float* transforms; const BoundingBox* sdfBoxes; const float* lines;
    const GlobalUbo* g;
    Stats* stats; ScratchHeader* header; Record* records; WorkItem* items;
    uint32_t drawCount, sdfBoxCount, lineCount, drawsCulled, transformCount, segmentCount, recordCapacity, chunksMax;
    uint64_t itemCapacity;
    int32_t width, height;
};

// edge e (0 .. 11) of the box {lo, hi}: axis a = e / 4, from the (e % 4)-th corner with bit a clear to that corner with bit a set
PLR_DI void boxEdge(const float* lo, const float* hi, uint32_t e, float* a, float* b) {
    const uint32_t axis = e >> 2, j = e & 3u;
    const uint32_t k = (j & ((1u << axis) - 1u)) | ((j >> axis) << (axis + 1u));
    for (uint32_t r = 0; r < 3u; r++) {
        a[r] = (k >> r) & 1u ? hi[r] : lo[r];
        b[r] = ((k | (1u << axis)) >> r) & 1u ? hi[r] : lo[r];
    }
}

__global__ __launch_bounds__(256) void debugGeometrySetupKernel(SetupParams p) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u;
    bool submitted = false, clipped = false, rejected = false, drawn = false;
    Record rec{};
    uint32_t chunks = 0;
    int32_t firstIndex = 0;
    if (s < p.segmentCount) {
        const uint32_t drawSegments = p.drawCount * kEdgesPerBox, boxSegments = drawSegments + p.sdfBoxCount * kEdgesPerBox;
        float a[3] = {0.f, 0.f, 0.f}, b[3] = {0.f, 0.f, 0.f}, rgb[3] = {0.f, 0.f, 0.f};
        if (s < drawSegments) {
            const uint32_t d = s / kEdgesPerBox;
            const prepass::Draw draw = p.draws[d];
            if (draw.transformIndex < p.transformCount && !(p.drawsCulled != 0u && draw.indexCount == 0u)) {
                const float* bd = p.bounds + (size_t)d * kBoundsFloats;
                const float* m = p.transforms + (size_t)draw.transformIndex * 48u; // model
                float lo[3], hi[3];
                for (uint32_t k = 0; k < 8u; k++) {
                    const float x = k & 1u ? bd[3] : bd[0], y = k & 2u ? bd[4] : bd[1], z = k & 4u ? bd[5] : bd[2];
                    for (int r = 0; r < 3; r++) {
                        const float c = prepass::clipComponent(m, r, x, y, z);
                        lo[r] = k == 0u ? c : (c < lo[r] ? c : lo[r]);
                        hi[r] = k == 0u ? c : (c > hi[r] ? c : hi[r]);
                    }
                }
                boxEdge(lo, hi, s - d * kEdgesPerBox, a, b);
                rgb[0] = kDrawBoxColor[0]; rgb[1] = kDrawBoxColor[1]; rgb[2] = kDrawBoxColor[2];
                submitted = true;
            }
        } else if (s < boxSegments) {
            const uint32_t i = (s - drawSegments) / kEdgesPerBox;
            const BoundingBox bb = p.sdfBoxes[i];
            boxEdge(bb.bbMin, bb.bbMax, (s - drawSegments) - i * kEdgesPerBox, a, b);
            rgb[0] = kSdfBoxColor[0]; rgb[1] = kSdfBoxColor[1]; rgb[2] = kSdfBoxColor[2];
            submitted = true;
        } else {
            const float* l = p.lines + (size_t)(s - boxSegments) * kLineFloats;
            for (int r = 0; r < 3; r++) { a[r] = l[r]; b[r] = l[3 + r]; rgb[r] = l[6 + r]; }
            submitted = true;
        }
        if (submitted) {
            const float* M = p.g->viewProjection;
            float A[4], B[4];
            for (int i = 0; i < 4; i++) { A[i] = prepass::clipComponent(M, i, a[0], a[1], a[2]); B[i] = prepass::clipComponent(M, i, b[0], b[1], b[2]); }
            for (int plane = 0; plane < prepass::kClipPlanes && !rejected; plane++) {
                const float da = prepass::planeDistance(plane, A[0], A[1], A[2], A[3]), db = prepass::planeDistance(plane, B[0], B[1], B[2], B[3]);
                const bool ina = da >= 0.f, inb = db >= 0.f; // (a NaN is outside)
                if (!ina && !inb) rejected = true;
                else if (ina != inb) { // from the inside end towards the outside one
                    clipped = true;
                    const float di = ina ? da : db, dout = ina ? db : da;
                    const float t = di / (di - dout);
                    for (int i = 0; i < 4; i++) {
                        const float in = ina ? A[i] : B[i], out = ina ? B[i] : A[i];
                        const float v = in + t * (out - in);
                        if (ina) B[i] = v; else A[i] = v;
                    }
                }
            }
            if (!rejected) {
                int32_t X0, Y0, X1, Y1;
                float z0, z1;
                const bool ok0 = prepass::projectAndSnap(A[0], A[1], A[2], A[3], (float)p.width, (float)p.height, &X0, &Y0, &z0);
                const bool ok1 = prepass::projectAndSnap(B[0], B[1], B[2], B[3], (float)p.width, (float)p.height, &X1, &Y1, &z1);
                if (!ok0 || !ok1) rejected = true;
                else {
                    const int32_t dX = X1 - X0, dY = Y1 - Y0; // |X|, |Y| <= 2^28
                    const bool yMajor = !((dX < 0 ? -dX : dX) >= (dY < 0 ? -dY : dY));
                    int32_t U0 = yMajor ? Y0 : X0, V0 = yMajor ? X0 : Y0, U1 = yMajor ? Y1 : X1, V1 = yMajor ? X1 : Y1;
                    if (U0 > U1) {
                        const int32_t tu = U0, tv = V0; U0 = U1; V0 = V1; U1 = tu; V1 = tv;
                        const float tz = z0; z0 = z1; z1 = tz;
                    }
                    const int32_t EU = yMajor ? p.height : p.width;
                    const int32_t i0 = max(0, (U0 + 127) >> 8), i1 = min(EU - 1, (U1 - 129) >> 8);
                    if (U1 - U0 > 0 && i1 >= i0) {
                        drawn = true;
                        firstIndex = i0;
                        chunks = min(((uint32_t)(i1 - i0) + kChunkSteps) / kChunkSteps, p.chunksMax);
                        rec.u0 = U0; rec.v0 = V0; rec.u1 = U1; rec.v1 = V1; rec.z0 = z0; rec.z1 = z1;
                        rec.color = packR11G11B10Exact(vec3(rgb[0], rgb[1], rgb[2]));
                        rec.sAndMajor = s | (yMajor ? 0x80000000u : 0u);
                    }
                }
            }
        }
    }
    // the counters, the record slots and the work items: ballots, pop-counts and a wave scan, one atomic add per wave and counter (every lane of the wave is here)
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long drawnMask = __ballot(drawn), submittedMask = __ballot(submitted), clippedMask = __ballot(clipped), rejectedMask = __ballot(rejected);
    uint32_t scan = chunks; // inclusive prefix sum of the chunk counts
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)scan, off);
        if ((int)lane >= off) scan += up;
    }
    const uint32_t waveItems = (uint32_t)__shfl((int)scan, 63);
    uint32_t recordBase = 0, itemBase = 0;
    if (lane == 0) {
        uint32_t* stats = (uint32_t*)p.stats;
        if (submittedMask) atomicAdd(stats + 0, (uint32_t)__popcll(submittedMask));
        if (clippedMask) atomicAdd(stats + 1, (uint32_t)__popcll(clippedMask));
        if (rejectedMask) atomicAdd(stats + 2, (uint32_t)__popcll(rejectedMask));
        if (drawnMask) {
            atomicAdd(stats + 3, (uint32_t)__popcll(drawnMask));
            recordBase = atomicAdd(&p.header->records, (uint32_t)__popcll(drawnMask));
            itemBase = atomicAdd(&p.header->items, waveItems);
        }
    }
    recordBase = (uint32_t)__shfl((int)recordBase, 0);
    itemBase = (uint32_t)__shfl((int)itemBase, 0);
    if (drawn) {
        const uint32_t slot = recordBase + (uint32_t)__popcll(drawnMask & below);
        if (slot < p.recordCapacity) {
            p.records[slot] = rec;
            const uint64_t at = (uint64_t)itemBase + (scan - chunks);
            for (uint32_t c = 0; c < p.chunksMax && c < chunks; c++)
                if (at + c < p.itemCapacity) p.items[at + c] = WorkItem{slot, (uint32_t)firstIndex + c * kChunkSteps};
        }
    }
}

struct RasterParams {
    const ScratchHeader* header; const Record* records; const WorkItem* items;
    unsigned long long* keys; uint32_t* color; float* depth; Stats* stats;
    uint32_t recordCapacity, itemLimit; // itemLimit = min(the list's capacity, 2^32 - 1): what the header's count is held to
    int32_t width, height;
};

// kResolve = false: launch A, the fragments' keys into the scratch; true: launch B, the winners' stores and the scratch back to 0
template <bool kResolve> __global__ __launch_bounds__(256) void debugGeometryRasterKernel(RasterParams p) {
    const uint32_t lane = threadIdx.x & 63u, waves = gridDim.x * 4u;
    const uint32_t itemCount = min(p.header->items, p.itemLimit), recordCount = min(p.header->records, p.recordCapacity);
    uint32_t counted = 0;
    for (uint32_t item = blockIdx.x * 4u + (threadIdx.x >> 6); item < itemCount; item += waves) {
        const WorkItem it = p.items[item];
        if (it.record >= recordCount) continue;
        const Record r = p.records[it.record];
        const bool yMajor = (r.sAndMajor >> 31) != 0u;
        const uint32_t s = r.sAndMajor & 0x7fffffffu;
        const int32_t EU = yMajor ? p.height : p.width, EV = yMajor ? p.width : p.height;
        const int32_t dU = r.u1 - r.u0, dV = r.v1 - r.v0;
        const int64_t i = (int64_t)it.firstStep + lane;
        const int32_t i0 = max(0, (r.u0 + 127) >> 8), i1 = min(EU - 1, (r.u1 - 129) >> 8);
        bool hit = false;
        if (dU > 0 && i >= i0 && i <= i1) {
            const int32_t c = 256 * (int32_t)i + 128;
            const int64_t num = (int64_t)r.v0 * dU + (int64_t)(c - r.u0) * dV, den = 256ll * dU;
            int64_t j = num / den;
            if (num % den != 0 && num < 0) j--; // floor
            if (j >= 0 && j < EV) {
                const double t = (double)(c - r.u0) / (double)dU;
                const float zf = (float)((double)r.z0 + t * ((double)r.z1 - (double)r.z0));
                const size_t pixel = yMajor ? (size_t)i * (size_t)p.width + (size_t)j : (size_t)j * (size_t)p.width + (size_t)i;
                const unsigned long long key = ((unsigned long long)f2u(zf) << 32) | (unsigned long long)(s + 1u);
                if (zf > 0.f) { // (a NaN fails)
                    if constexpr (!kResolve) {
                        if (zf >= p.depth[pixel]) {
                            atomicMax(p.keys + pixel, key);
                            hit = true;
                        }
                    } else if (p.keys[pixel] == key) {
                        p.color[pixel] = r.color;
                        p.depth[pixel] = zf;
                        p.keys[pixel] = 0ull;
                        hit = true;
                    }
                }
            }
        }
        counted += (uint32_t)__popcll(__ballot(hit));
    }
    if (lane == 0 && counted) atomicAdd(kResolve ? &p.stats->pixelsWritten : &p.stats->fragments, counted);
}

// what the launcher knows about the pass's scratch (PassScratch): from which byte on it may hold something else than zeros - the header, the records and the
// work list of the last execution lie behind the keys of its frame size -, and whether an execution got as far as its last launch
struct ScratchBookkeeping : ScratchState {
    size_t dirtyFrom = ~(size_t)0;
    bool keysClean = true;
};

static int launchDebugGeometry(const PassCtx& c) {
    if (c.push.size() != sizeof(PushConstants)) return c.fail(-1, "debugGeometry: push constants {drawCount, sdfBoxCount, lineCount, drawsCulled} missing (16 bytes)");
    PushConstants pc{};
    std::memcpy(&pc, c.push.data(), sizeof(pc));
    if (c.dispatch[0] != 1u || c.dispatch[1] != 1u || c.dispatch[2] != 1u || c.base[0] != 0u || c.base[1] != 0u)
        return c.fail(-1, "debugGeometry: the dispatch is {1, 1, 1} (the launcher derives its grids from the push constants)");
    if (pc.drawsCulled > 1u) return c.fail(-1, "debugGeometry: drawsCulled is " + std::to_string(pc.drawsCulled) + ", it must be 0 or 1");
    const uint64_t segments = segmentCount(pc.drawCount, pc.sdfBoxCount, pc.lineCount);
    if (segments > kMaxSegments) return c.fail(-1, "debugGeometry: " + std::to_string(segments) + " segments, at most " + std::to_string(kMaxSegments) + " have a number");
    if (int rc = c.needGlobal()) return rc;
    if (int rc = c.needStorage(kColorBinding, F_R11G11B10, "debugGeometry colour")) return rc;
    if (int rc = c.needStorage(kDepthBinding, F_D32, "debugGeometry depth")) return rc;
    const ImgView color = c.storage[kColorBinding], depth = c.storage[kDepthBinding];
    if (color.w != depth.w || color.h != depth.h)
        return c.fail(-4, "debugGeometry: colour is " + std::to_string(color.w) + " x " + std::to_string(color.h) + " and depth " + std::to_string(depth.w) + " x " + std::to_string(depth.h) + ": they must have one size");
    if (color.w < 1 || color.h < 1 || color.w > prepass::kMaxResolution || color.h > prepass::kMaxResolution)
        return c.fail(-4, "debugGeometry: the images are " + std::to_string(color.w) + " x " + std::to_string(color.h) + ", each side must be 1 .. " + std::to_string(prepass::kMaxResolution));
    if (color.ptr == depth.ptr) return c.fail(-4, "debugGeometry: colour and depth are the same image");
    if (pc.drawCount) {
        if (int rc = c.needSbuf(kDrawBinding, (size_t)pc.drawCount * sizeof(prepass::Draw), "debugGeometry draws (24 bytes per draw)")) return rc;
        if (int rc = c.needSbuf(kBoundsBinding, (size_t)pc.drawCount * kBoundsFloats * sizeof(float), "debugGeometry bounds (6 floats per draw: lo.xyz, hi.xyz)")) return rc;
        if (int rc = c.needSbuf(kTransformBinding, 0, "debugGeometry transforms (MainPassMatrices[]: model, mvp, mvpPrevious)")) return rc;
    }
    if (pc.sdfBoxCount)
        if (int rc = c.needSbuf(kSdfBoxBinding, (size_t)pc.sdfBoxCount * sizeof(BoundingBox), "debugGeometry sdfBoxes (32 bytes per box: min.xyz, pad, max.xyz, pad)")) return rc;
    if (pc.lineCount)
        if (int rc = c.needSbuf(kLineBinding, (size_t)pc.lineCount * kLineFloats * sizeof(float), "debugGeometry lines (9 floats per line: a.xyz, b.xyz, rgb)")) return rc;
    if (int rc = c.needSbuf(kStatsBinding, sizeof(Stats), "debugGeometry stats (32 bytes)")) return rc;
    if (c.sbuf[kStatsBinding].readOnly) return c.fail(-4, "debugGeometry: the stats buffer (binding " + std::to_string(kStatsBinding) + ") is bound read-only");
    for (int in = 0; in < kStatsBinding; in++)
        if (c.hasSbuf(in) && c.sbuf[in].ptr == c.sbuf[kStatsBinding].ptr)
            return c.fail(-4, "debugGeometry: the stats buffer is also bound as an input (binding " + std::to_string(in) + ")");
    if (hipMemsetAsync(c.sbuf[kStatsBinding].ptr, 0, sizeof(Stats), c.stream) != hipSuccess) return c.fail(-2, "debugGeometry: clearing the counters failed");
    if (segments == 0u) return 0;

    const uint32_t width = (uint32_t)color.w, height = (uint32_t)color.h, chunksMax = chunksPerSegment(width, height);
    const uint64_t itemCapacity = segments * chunksMax;
    const size_t keys = keyBytes(width, height), headerAt = keys, recordsAt = headerAt + sizeof(ScratchHeader), itemsAt = recordsAt + (size_t)segments * sizeof(Record);
    const size_t total = itemsAt + (size_t)itemCapacity * sizeof(WorkItem);
    uint8_t* scratch = (uint8_t*)c.scratch(total); // zero-filled when it is (re)allocated, which also drops the bookkeeping
    if (!scratch) return c.fail(-2, "debugGeometry: cannot allocate " + std::to_string(total) + " bytes of scratch memory");
    ScratchBookkeeping* book = c.scratchState<ScratchBookkeeping>();
    if (!book) return -1;
    if (!book->keysClean) book->dirtyFrom = 0; // an execution that failed between its launches may have left keys behind
    if (keys > book->dirtyFrom && hipMemsetAsync(scratch + book->dirtyFrom, 0, keys - book->dirtyFrom, c.stream) != hipSuccess)
        return c.fail(-2, "debugGeometry: clearing the key scratch failed");
    book->dirtyFrom = keys;
    book->keysClean = false;
    if (hipMemsetAsync(scratch + headerAt, 0, sizeof(ScratchHeader), c.stream) != hipSuccess) return c.fail(-2, "debugGeometry: clearing the scratch header failed");

    SetupParams sp{};
    sp.draws = pc.drawCount ? (const prepass::Draw*)c.sbuf[kDrawBinding].ptr : nullptr; sp.bounds = pc.drawCount ? (const float*)c.sbuf[kBoundsBinding].ptr : nullptr;
    sp.transforms = pc.drawCount ? (const float*)c.sbuf[kTransformBinding].ptr : nullptr;
    sp.sdfBoxes = pc.sdfBoxCount ? (const BoundingBox*)c.sbuf[kSdfBoxBinding].ptr : nullptr; sp.lines = pc.lineCount ? (const float*)c.sbuf[kLineBinding].ptr : nullptr;
    sp.g = c.global; sp.stats = (Stats*)c.sbuf[kStatsBinding].ptr;
    sp.header = (ScratchHeader*)(scratch + headerAt); sp.records = (Record*)(scratch + recordsAt); sp.items = (WorkItem*)(scratch + itemsAt);
    sp.drawCount = pc.drawCount; sp.sdfBoxCount = pc.sdfBoxCount; sp.lineCount = pc.lineCount; sp.drawsCulled = pc.drawsCulled;
    sp.transformCount = pc.drawCount ? (uint32_t)std::min<size_t>(c.sbuf[kTransformBinding].size / sizeof(prepass::MainPassMatrices), 0xffffffffu) : 0u;
    sp.segmentCount = (uint32_t)segments; sp.recordCapacity = (uint32_t)segments; sp.chunksMax = chunksMax; sp.itemCapacity = itemCapacity;
    sp.width = color.w; sp.height = color.h;
    debugGeometrySetupKernel<<<divUp((uint32_t)segments, 256u), 256, 0, c.stream>>>(sp);
    PLR_CHECK_LAUNCH(c);

    RasterParams rp{};
    rp.header = sp.header; rp.records = sp.records; rp.items = sp.items;
    rp.keys = (unsigned long long*)scratch; rp.color = (uint32_t*)color.ptr; rp.depth = (float*)depth.ptr; rp.stats = sp.stats;
    rp.recordCapacity = sp.recordCapacity; rp.itemLimit = (uint32_t)std::min<uint64_t>(itemCapacity, 0xffffffffull);
    rp.width = color.w; rp.height = color.h;
    // a persistent grid over the work list: a wave per item, at most 8 blocks of 4 waves per CU of the 256
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((itemCapacity + 3u) / 4u, 2048u);
    debugGeometryRasterKernel<false><<<blocks, 256, 0, c.stream>>>(rp);
    PLR_CHECK_LAUNCH(c);
    debugGeometryRasterKernel<true><<<blocks, 256, 0, c.stream>>>(rp);
    PLR_CHECK_LAUNCH(c);
    book->keysClean = true;
    return 0;
}

} // namespace debuggeo
static int debug_geometry_launch(const PassCtx& c) { return debuggeo::launchDebugGeometry(c); }
static int debug_geometry_launch_fast(const PassCtx& c) { return debuggeo::launchDebugGeometry(c); }
PLR_REGISTER_SHADER("debugGeometry.comp", debug_geometry_launch);
PLR_REGISTER_SHADER_FAST("debugGeometry.comp", debug_geometry_launch_fast);
} // namespace plr
