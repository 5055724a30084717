// "blueNoiseVoidAndCluster.comp" and "perlinNoise3D.comp": the frame's noise textures as compute passes - generateBlueNoiseTexture (Common/Noise.cpp:232-300,
// called for noise0 .. noise3 at RenderFrontend.cpp:1251-1269) and generate3DPerlinNoise (Noise.cpp:422-497, Volumetrics.cpp:71-90), with the two host tables
// plr_noise_gaussian_table and plr_noise_perlin_gradients (DESIGN.md "Noise textures as compute passes"; plrf_generate_noise). Both kernel sets run these kernels:
// every output byte is decided by a written contract in integers and IEEE fp32. This file is built with the exact set's flags (no contraction, denormals kept,
// correctly rounded division).
//
// THE BLUE NOISE CONTRACT, one channel of a W x H texture (N = W H, 4 <= W, H <= 64, index = y W + x), stream s = firstStream + channel:
//   key        lowbias32(seed ^ (0x9E3779B9u (s + 1)))                                           (device/noise.h holds the integer functions)
//   white[i]   lowbias32(key + i) & 255
//   ones       uint32(float(N) * 0.1f)
//   binarise   256-bin histogram; t = the first threshold with float(cum[t]) / float(N) >= float(ones) / float(N); pattern = white <= t; then, in index order,
//              every set entry beyond the first `ones` is cleared
//   influence  of (x0, y0) on (x, y): G[((y - y0) mod H) W + ((x - x0) mod W)], G the table at binding 1
//   LUT        fp32 per pixel. A fresh LUT adds the influences of the minority pixels in index order, starting from 0.f; every later update is ONE fp32 add or
//              subtract per pixel
//   cluster    the minority pixel with the largest LUT value, the lowest index on a tie; void: the majority pixel with the smallest, the lowest index on a tie
//   prototype  fresh LUT; at most N times: remove the tightest cluster c, subtract its influence, find the biggest void v; v == c: restore c, converged, stop;
//              else set v, add its influence, swaps += 1. N swaps without converging: stop, converged stays 0
//   ranks      fresh LUT of the prototype; rank ones - 1 .. 0: remove the tightest cluster, subtract, it takes the rank; then from the prototype and its fresh LUT
//              again, rank ones .. N - 1: set the biggest void, add, it takes the rank
//   code       uint8((float(rank) + 0.5f) / float(N) * 255.f), stored at byte (y W + x) channels + channel; status[4 channel ..] = {swaps, converged, ones, 0}
// One block of 1024 lanes per channel. Lane i owns pixels i, i + 1024, ... (at most four): their LUT values, pattern bits and ranks live in its registers. G sits
// in LDS. A step is one block-wide (value, index) reduction - wave shuffles, then the 16 wave results through LDS, read back by every lane, so that the
// chosen pixel is known to all after ONE barrier (the 16 slots alternate between two halves: a lane that runs ahead writes the other half) - and one add or
// subtract per owned pixel. The pattern is also kept as a bitmask in LDS, which the fresh LUT walks in index order. Every loop is bounded by N, `ones` or a
// constant: nothing can spin.
//
// THE PERLIN CONTRACT, voxel (x, y, z) of an R^3 volume (index = x + y R + z R^2), g = gridCellCount, gradients at binding 1 (cell (x, y, z): (x g + y) g + z):
//   uv = float(coord) / float(R); s = uv * float(g); cell = int(s); residual = float(g) * uv - float(cell)                                    (per axis)
//   dot(corner k) = (G.x o.x + G.y o.y) + G.z o.z with G the gradient of cell ((cell + k) % g per axis) and o = residual - float(k)
//   mix(a, b, t) = a * (1.f - t) + b * t along z, then y, then x, with the RESIDUAL as the weight (Noise.cpp:473-481: the smoothstep is computed and not used)
//   value / sqrt(3 / 4.f) (= 0x3f5db3d7), * 0.5f + 0.5f, clamped to [0, 1], uint8(value * 255.f)
#include <cmath>

#include "../../../include/plr.h"
#include "../backend.h"
#include "../device/noise.h"

namespace plr {
namespace noise {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kWaves = kBlueThreads / 64u;

struct BlueParams {
    uint8_t* image;
    const float* table;
    uint32_t* status;
    uint32_t width, height, channels, seed, firstStream;
};

// candidate a (value, index) beats b: kNone is no candidate; the lowest index wins a tie, so the order of the comparisons cannot matter
template <bool Cluster> PLR_DI bool beats(float av, uint32_t ai, float bv, uint32_t bi) {
    if (ai == kNone) return false;
    if (bi == kNone) return true;
    if (Cluster ? av > bv : av < bv) return true;
    return av == bv && ai < bi;
}

// the tightest cluster (Cluster) or the biggest void of the block's pattern, in every lane; kNone if there is no such pixel
template <bool Cluster>
PLR_DI uint32_t selectPixel(const float (&lut)[kBluePixelsPerThread], uint32_t mine, uint32_t n, float* slotValue, uint32_t* slotIndex, uint32_t& half) {
    float bv = 0.f;
    uint32_t bi = kNone;
#pragma unroll
    for (uint32_t k = 0; k < kBluePixelsPerThread; k++) {
        const uint32_t p = threadIdx.x + k * kBlueThreads;
        if (p < n && ((mine >> k) & 1u) == (Cluster ? 1u : 0u) && beats<Cluster>(lut[k], p, bv, bi)) { bv = lut[k]; bi = p; }
    }
#pragma unroll
    for (int offset = 32; offset > 0; offset >>= 1) {
        const float ov = __shfl_xor(bv, offset);
        const uint32_t oi = (uint32_t)__shfl_xor((int)bi, offset);
        if (beats<Cluster>(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    float* values = slotValue + half * kWaves;
    uint32_t* indices = slotIndex + half * kWaves;
    if ((threadIdx.x & 63u) == 0u) { values[threadIdx.x >> 6] = bv; indices[threadIdx.x >> 6] = bi; }
    __syncthreads();
    bv = values[0]; bi = indices[0];
#pragma unroll
    for (uint32_t w = 1; w < kWaves; w++)
        if (beats<Cluster>(values[w], indices[w], bv, bi)) { bv = values[w]; bi = indices[w]; }
    half ^= 1u;
    return bi;
}

struct OwnedPixels { uint32_t x[kBluePixelsPerThread], y[kBluePixelsPerThread]; };

// lut += or -= the influence of pixel `source` on the lane's pixels: one fp32 operation each
template <bool Add>
PLR_DI void applyInfluence(float (&lut)[kBluePixelsPerThread], const OwnedPixels& own, uint32_t source, uint32_t w, uint32_t h, uint32_t n, const float* table) {
    const uint32_t y0 = source / w, x0 = source - y0 * w;
#pragma unroll
    for (uint32_t k = 0; k < kBluePixelsPerThread; k++) {
        if (threadIdx.x + k * kBlueThreads >= n) continue;
        const uint32_t dx = own.x[k] >= x0 ? own.x[k] - x0 : own.x[k] + w - x0;
        const uint32_t dy = own.y[k] >= y0 ? own.y[k] - y0 : own.y[k] + h - y0;
        const float g = table[dy * w + dx];
        lut[k] = Add ? lut[k] + g : lut[k] - g;
    }
}

// calculateFilterLut: the minority pixels of the LDS bitmask in index order, from 0.f
PLR_DI void freshLut(float (&lut)[kBluePixelsPerThread], const OwnedPixels& own, const uint32_t* mask, uint32_t w, uint32_t h, uint32_t n, const float* table) {
    __syncthreads(); // the owners' updates of the bitmask
#pragma unroll
    for (uint32_t k = 0; k < kBluePixelsPerThread; k++) lut[k] = 0.f;
    for (uint32_t word = 0; word < (n + 31u) / 32u; word++) {
        const uint32_t bits = mask[word];
        if (bits == 0u) continue;
        for (uint32_t b = 0; b < 32u; b++)
            if ((bits >> b) & 1u) applyInfluence<true>(lut, own, word * 32u + b, w, h, n, table);
    }
}

PLR_DI void setOwned(uint32_t pixel, bool value, uint32_t& mine, uint32_t* mask) {
    if ((pixel & (kBlueThreads - 1u)) != threadIdx.x) return;
    const uint32_t k = pixel / kBlueThreads;
    if (value) { mine |= 1u << k; if (mask) atomicOr(&mask[pixel >> 5], 1u << (pixel & 31u)); }
    else { mine &= ~(1u << k); if (mask) atomicAnd(&mask[pixel >> 5], ~(1u << (pixel & 31u))); }
}

__global__ void __launch_bounds__(kBlueThreads) blueNoiseVoidAndClusterKernel(BlueParams p) {
    __shared__ float table[kBlueMaxSize * kBlueMaxSize];
    __shared__ uint32_t mask[kBlueMaxSize * kBlueMaxSize / 32u];
    __shared__ uint32_t histogram[256];
    __shared__ float slotValue[2u * kWaves];
    __shared__ uint32_t slotIndex[2u * kWaves];
    const uint32_t tid = threadIdx.x, channel = blockIdx.x;
    const uint32_t w = p.width, h = p.height, n = w * h; // (the launcher checked 4 <= w, h <= 64: n <= 4096 = the LDS table, 4 pixels per lane)
    const uint32_t key = streamKey(p.seed, p.firstStream + channel);
    const uint32_t ones = minorityCount(n);
    for (uint32_t i = tid; i < n; i += kBlueThreads) table[i] = p.table[i];
    if (tid < 256u) histogram[tid] = 0u;
    if (tid < kBlueMaxSize * kBlueMaxSize / 32u) mask[tid] = 0u;
    __syncthreads();
    OwnedPixels own;
    uint32_t white[kBluePixelsPerThread];
#pragma unroll
    for (uint32_t k = 0; k < kBluePixelsPerThread; k++) {
        const uint32_t pixel = tid + k * kBlueThreads;
        own.x[k] = own.y[k] = white[k] = 0u;
        if (pixel >= n) continue;
        own.y[k] = pixel / w; own.x[k] = pixel - own.y[k] * w;
        white[k] = whiteNoise(key, pixel);
        atomicAdd(&histogram[white[k]], 1u);
    }
    __syncthreads();
    // binarizeArray: every lane walks the histogram to the same threshold
    uint32_t threshold = 0u, cumulative = 0u;
    const float target = (float)ones / (float)n;
    for (uint32_t t = 0; t < 256u; t++) {
        cumulative += histogram[t];
        if ((float)cumulative / (float)n >= target) { threshold = t; break; }
    }
#pragma unroll
    for (uint32_t k = 0; k < kBluePixelsPerThread; k++) {
        const uint32_t pixel = tid + k * kBlueThreads;
        if (pixel < n && white[k] <= threshold) atomicOr(&mask[pixel >> 5], 1u << (pixel & 31u));
    }
    __syncthreads();
    // a set pixel stays if fewer than `ones` set pixels come before it in index order
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kBluePixelsPerThread; k++) {
        const uint32_t pixel = tid + k * kBlueThreads;
        if (pixel >= n || ((mask[pixel >> 5] >> (pixel & 31u)) & 1u) == 0u) continue;
        uint32_t before = (uint32_t)__popc(mask[pixel >> 5] & ((1u << (pixel & 31u)) - 1u));
        for (uint32_t word = 0; word < (pixel >> 5); word++) before += (uint32_t)__popc(mask[word]);
        if (before < ones) mine |= 1u << k;
    }
    __syncthreads();
    if (tid < kBlueMaxSize * kBlueMaxSize / 32u) mask[tid] = 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kBluePixelsPerThread; k++)
        if ((mine >> k) & 1u) atomicOr(&mask[(tid + k * kBlueThreads) >> 5], 1u << ((tid + k * kBlueThreads) & 31u));

    float lut[kBluePixelsPerThread];
    uint32_t half = 0u;
    freshLut(lut, own, mask, w, h, n, table);
    // createPrototypeBinaryPattern: swap the tightest cluster with the biggest void until the removed pixel is the void itself, N swaps at the most
    uint32_t swaps = 0u, converged = 0u;
    for (uint32_t iteration = 0; iteration < n; iteration++) {
        const uint32_t removed = selectPixel<true>(lut, mine, n, slotValue, slotIndex, half);
        if (removed >= n) break; // (no minority pixel: cannot happen with ones >= 1; the loop still ends)
        setOwned(removed, false, mine, mask);
        applyInfluence<false>(lut, own, removed, w, h, n, table);
        const uint32_t added = selectPixel<false>(lut, mine, n, slotValue, slotIndex, half);
        if (added >= n) break;
        if (added == removed) { setOwned(removed, true, mine, mask); converged = 1u; break; }
        setOwned(added, true, mine, mask);
        applyInfluence<true>(lut, own, added, w, h, n, table);
        swaps++;
    }
    // generateBlueNoiseTexture: both rank phases start from the prototype and its fresh LUT
    freshLut(lut, own, mask, w, h, n, table);
    const uint32_t prototype = mine;
    float prototypeLut[kBluePixelsPerThread];
    uint32_t rank[kBluePixelsPerThread];
#pragma unroll
    for (uint32_t k = 0; k < kBluePixelsPerThread; k++) { prototypeLut[k] = lut[k]; rank[k] = 0u; }
    for (uint32_t r = ones; r-- > 0u;) {
        const uint32_t removed = selectPixel<true>(lut, mine, n, slotValue, slotIndex, half);
        if (removed >= n) break;
        setOwned(removed, false, mine, nullptr);
        applyInfluence<false>(lut, own, removed, w, h, n, table);
        if ((removed & (kBlueThreads - 1u)) == tid) rank[removed / kBlueThreads] = r;
    }
    mine = prototype;
#pragma unroll
    for (uint32_t k = 0; k < kBluePixelsPerThread; k++) lut[k] = prototypeLut[k];
    for (uint32_t r = ones; r < n; r++) {
        const uint32_t added = selectPixel<false>(lut, mine, n, slotValue, slotIndex, half);
        if (added >= n) break;
        setOwned(added, true, mine, nullptr);
        applyInfluence<true>(lut, own, added, w, h, n, table);
        if ((added & (kBlueThreads - 1u)) == tid) rank[added / kBlueThreads] = r;
    }
#pragma unroll
    for (uint32_t k = 0; k < kBluePixelsPerThread; k++) {
        const uint32_t pixel = tid + k * kBlueThreads;
        if (pixel < n) p.image[(size_t)pixel * p.channels + channel] = (uint8_t)rankCode(rank[k], n);
    }
    if (tid == 0u) {
        uint32_t* s = p.status + (size_t)channel * kBlueStatusWords;
        s[0] = swaps; s[1] = converged; s[2] = ones; s[3] = 0u;
    }
}

static int launchBlueNoise(const PassCtx& c) {
    if (c.push.size() != sizeof(BluePushConstants)) return c.fail(-1, "blueNoiseVoidAndCluster: push constants {seed, firstStream} missing");
    BluePushConstants pc{};
    std::memcpy(&pc, c.push.data(), sizeof(pc));
    if (!c.hasStorage(kBlueImageBinding)) return c.fail(PLR_ERR_BINDING, "blueNoiseVoidAndCluster: missing storage image at binding 0 (the R8 or RG8 texture to fill)");
    const ImgView& img = c.storage[kBlueImageBinding];
    if (img.fmt != F_R8 && img.fmt != F_RG8) return c.fail(PLR_ERR_BINDING, "blueNoiseVoidAndCluster: the image at binding 0 is neither R8 nor RG8");
    if (img.d > 1) return c.fail(PLR_ERR_BINDING, "blueNoiseVoidAndCluster: the image at binding 0 is not two-dimensional");
    if (img.w < (int)kBlueMinSize || img.w > (int)kBlueMaxSize || img.h < (int)kBlueMinSize || img.h > (int)kBlueMaxSize)
        return c.fail(-1, "blueNoiseVoidAndCluster: the image is " + std::to_string(img.w) + " x " + std::to_string(img.h) + ", a size outside 4 .. 64");
    const uint32_t channels = img.fmt == F_R8 ? 1u : 2u;
    if (c.dispatch[0] != channels || c.dispatch[1] != 1u || c.dispatch[2] != 1u || c.base[0] != 0u || c.base[1] != 0u || c.base[2] != 0u)
        return c.fail(-1, "blueNoiseVoidAndCluster: the dispatch is {channels, 1, 1}, one block per channel of the image's format (R8: 1, RG8: 2)");
    const size_t pixels = (size_t)img.w * (size_t)img.h;
    if (int rc = c.needSbuf(kBlueTableBinding, pixels * sizeof(float), "blueNoiseVoidAndCluster Gaussian table (binding 1: width height floats, plr_noise_gaussian_table)")) return rc;
    if (int rc = c.needSbuf(kBlueStatusBinding, (size_t)channels * kBlueStatusWords * sizeof(uint32_t), "blueNoiseVoidAndCluster status (binding 2: {swaps, converged, ones, 0} per channel)")) return rc;
    if (c.sbuf[kBlueStatusBinding].readOnly) return c.fail(PLR_ERR_BINDING, "blueNoiseVoidAndCluster: the status buffer (binding 2) is bound read-only");
    if (c.sbuf[kBlueStatusBinding].ptr == c.sbuf[kBlueTableBinding].ptr) return c.fail(PLR_ERR_BINDING, "blueNoiseVoidAndCluster: the status buffer is also bound as the Gaussian table");
    BlueParams p{};
    p.image = (uint8_t*)img.ptr; p.table = (const float*)c.sbuf[kBlueTableBinding].ptr; p.status = (uint32_t*)c.sbuf[kBlueStatusBinding].ptr;
    p.width = (uint32_t)img.w; p.height = (uint32_t)img.h; p.channels = channels; p.seed = pc.seed; p.firstStream = pc.firstStream;
    blueNoiseVoidAndClusterKernel<<<channels, kBlueThreads, 0, c.stream>>>(p);
    PLR_CHECK_LAUNCH(c);
    return 0;
}

// ---- "perlinNoise3D.comp"
struct PerlinParams {
    uint8_t* image;
    const float4* gradients;
    uint32_t resolution, cells;
};

PLR_DI float cornerDot(const PerlinParams& p, const int (&cell)[3], const float (&residual)[3], int cx, int cy, int cz) {
    const int g = (int)p.cells;
    const float4 gradient = p.gradients[(((cell[0] + cx) % g) * g + (cell[1] + cy) % g) * g + (cell[2] + cz) % g];
    const float ox = residual[0] - (float)cx, oy = residual[1] - (float)cy, oz = residual[2] - (float)cz;
    return (gradient.x * ox + gradient.y * oy) + gradient.z * oz;
}
PLR_DI float mixOf(float a, float b, float t) { return a * (1.f - t) + b * t; }

__global__ void __launch_bounds__(kPerlinThreads) perlinNoise3DKernel(PerlinParams p) {
    const uint32_t r = p.resolution, i = blockIdx.x * kPerlinThreads + threadIdx.x; // (r <= 256: r^3 <= 2^24)
    if (i >= r * r * r) return;
    const uint32_t coord[3] = {i % r, (i / r) % r, i / (r * r)};
    const float fr = (float)r, fg = (float)p.cells;
    int cell[3];
    float residual[3];
    for (int a = 0; a < 3; a++) {
        const float uv = (float)coord[a] / fr;
        cell[a] = (int)(uv * fg);
        residual[a] = fg * uv - (float)cell[a];
    }
    const float i00 = mixOf(cornerDot(p, cell, residual, 0, 0, 0), cornerDot(p, cell, residual, 0, 0, 1), residual[2]);
    const float i01 = mixOf(cornerDot(p, cell, residual, 0, 1, 0), cornerDot(p, cell, residual, 0, 1, 1), residual[2]);
    const float i10 = mixOf(cornerDot(p, cell, residual, 1, 0, 0), cornerDot(p, cell, residual, 1, 0, 1), residual[2]);
    const float i11 = mixOf(cornerDot(p, cell, residual, 1, 1, 0), cornerDot(p, cell, residual, 1, 1, 1), residual[2]);
    float value = mixOf(mixOf(i00, i01, residual[1]), mixOf(i10, i11, residual[1]), residual[0]);
    value = value / __uint_as_float(0x3f5db3d7u); // sqrt(3 / 4.f), correctly rounded
    value = value * 0.5f + 0.5f;
    value = value < 0.f ? 0.f : (value > 1.f ? 1.f : value);
    p.image[i] = (uint8_t)(value * 255.f);
}

static int launchPerlinNoise(const PassCtx& c) {
    if (c.push.size() != sizeof(PerlinPushConstants)) return c.fail(-1, "perlinNoise3D: push constant {gridCellCount} missing");
    PerlinPushConstants pc{};
    std::memcpy(&pc, c.push.data(), sizeof(pc));
    if (pc.gridCellCount < 1u || pc.gridCellCount > kPerlinMaxCells) return c.fail(-1, "perlinNoise3D: gridCellCount is " + std::to_string(pc.gridCellCount) + ", it must be 1 .. 32");
    if (int rc = c.needStorage(kPerlinImageBinding, F_R8, "perlinNoise3D volume")) return rc;
    const ImgView& img = c.storage[kPerlinImageBinding];
    if (img.w < 1 || img.w > (int)kPerlinMaxResolution || img.h != img.w || img.d != img.w)
        return c.fail(-1, "perlinNoise3D: the volume is " + std::to_string(img.w) + " x " + std::to_string(img.h) + " x " + std::to_string(img.d) + ", it must be a cube of 1 .. 256");
    const uint32_t r = (uint32_t)img.w, blocks = divUp(r * r * r, kPerlinThreads);
    if (c.dispatch[0] != blocks || c.dispatch[1] != 1u || c.dispatch[2] != 1u || c.base[0] != 0u || c.base[1] != 0u || c.base[2] != 0u)
        return c.fail(-1, "perlinNoise3D: the dispatch is {ceil(resolution^3 / 256), 1, 1}: a lane per voxel");
    const size_t cells = (size_t)pc.gridCellCount * pc.gridCellCount * pc.gridCellCount;
    if (int rc = c.needSbuf(kPerlinGradientBinding, cells * 4u * sizeof(float), "perlinNoise3D gradients (binding 1: gridCellCount^3 x 4 floats, plr_noise_perlin_gradients)")) return rc;
    if (((uintptr_t)c.sbuf[kPerlinGradientBinding].ptr & 15u) != 0u) return c.fail(PLR_ERR_BINDING, "perlinNoise3D: the gradients (binding 1) are not at a 16-byte address");
    PerlinParams p{};
    p.image = (uint8_t*)img.ptr; p.gradients = (const float4*)c.sbuf[kPerlinGradientBinding].ptr; p.resolution = r; p.cells = pc.gridCellCount;
    perlinNoise3DKernel<<<blocks, kPerlinThreads, 0, c.stream>>>(p);
    PLR_CHECK_LAUNCH(c);
    return 0;
}

} // namespace noise

static int blue_noise_launch(const PassCtx& c) { return noise::launchBlueNoise(c); }
static int blue_noise_launch_fast(const PassCtx& c) { return noise::launchBlueNoise(c); }
static int perlin_noise_launch(const PassCtx& c) { return noise::launchPerlinNoise(c); }
static int perlin_noise_launch_fast(const PassCtx& c) { return noise::launchPerlinNoise(c); }
PLR_REGISTER_SHADER("blueNoiseVoidAndCluster.comp", blue_noise_launch);
PLR_REGISTER_SHADER_FAST("blueNoiseVoidAndCluster.comp", blue_noise_launch_fast);
PLR_REGISTER_SHADER("perlinNoise3D.comp", perlin_noise_launch);
PLR_REGISTER_SHADER_FAST("perlinNoise3D.comp", perlin_noise_launch_fast);
} // namespace plr

// ---- the two tables: host code, no GPU
extern "C" int plr_noise_gaussian_table(uint32_t width, uint32_t height, float* out) {
    using namespace plr::noise;
    if (!out) return plr::setLastError(PLR_ERR_INVALID_ARGUMENT, "plr_noise_gaussian_table: out is null");
    if (width < kBlueMinSize || width > kBlueMaxSize || height < kBlueMinSize || height > kBlueMaxSize)
        return plr::setLastError(PLR_ERR_INVALID_ARGUMENT, "plr_noise_gaussian_table: " + std::to_string(width) + " x " + std::to_string(height) + " is a size outside 4 .. 64");
    for (uint32_t dy = 0; dy < height; dy++)
        for (uint32_t dx = 0; dx < width; dx++) {
            const uint32_t ox = dx < width - dx ? dx : width - dx, oy = dy < height - dy ? dy : height - dy;
            const float argument = -(float)(ox * ox + oy * oy) / (2.f * (1.9f * 1.9f)); // fp32; gaussianFilter, Noise.cpp:80-85
            out[dy * width + dx] = (float)std::exp((double)argument);                    // exp in double, one rounding
        }
    return PLR_OK;
}

extern "C" int plr_noise_perlin_gradients(uint32_t seed, uint32_t grid_cell_count, float* out) {
    using namespace plr::noise;
    if (!out) return plr::setLastError(PLR_ERR_INVALID_ARGUMENT, "plr_noise_perlin_gradients: out is null");
    if (grid_cell_count < 1u || grid_cell_count > kPerlinMaxCells)
        return plr::setLastError(PLR_ERR_INVALID_ARGUMENT, "plr_noise_perlin_gradients: grid_cell_count is " + std::to_string(grid_cell_count) + ", it must be 1 .. 32");
    const uint32_t key = streamKey(seed, kPerlinStream), cells = grid_cell_count * grid_cell_count * grid_cell_count;
    for (uint32_t cell = 0; cell < cells; cell++) {
        const double rx = (double)perlinAngle(lowbias32(key + 2u * cell)), ry = (double)perlinAngle(lowbias32(key + 2u * cell + 1u));
        out[4u * cell] = (float)(std::sin(rx) * std::cos(ry));
        out[4u * cell + 1u] = (float)(std::sin(rx) * std::sin(rx)); // the repeated sin rx is the reference's (Noise.cpp:444)
        out[4u * cell + 2u] = (float)std::cos(rx);
        out[4u * cell + 3u] = 0.f;
    }
    return PLR_OK;
}
