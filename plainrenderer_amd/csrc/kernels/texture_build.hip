// "textureMipChain.comp" and "textureBlockEncode.comp": the scene's texture store built on the GPU - the mip chain of appendMipChain (frontend/scene_packing.cpp)
// and a range-fit BC1 / BC3 / BC5 encoder as two compute passes (DESIGN.md "Texture store built on the GPU"; plrf_build_scene_textures). Both kernel sets run these
// kernels: every output byte is decided by a written integer contract (device/texture_build.h holds the arithmetic, one text for these kernels and the host's
// plr_encode_rgba8_to_bc).
//
// Both passes index their grid through a job table: job j owns the workgroups [jobs[j].firstGroup, jobs[j + 1].firstGroup), found by a binary search that is uniform
// over the workgroup. Every word address is checked against its buffer's word count before the access: a read outside gives 0, a write outside is dropped.
//   textureMipChain     a lane per texel of the level built: the four taps of the chain rule - two 8-byte loads where the pair is aligned, through blockTexel
//                       (device/bc_decode.h) where the level below is compressed -, the byte means two bytes at a time, one 4-byte store; neighbouring lanes write
//                       neighbouring words
//   textureBlockEncode  a lane per block: its four rows as 16-byte loads where the row lies inside the level at a 16-byte address, through the clamped path at the
//                       edges; the 16 texels stay in registers; one 8-byte (BC1) or 16-byte store, neighbouring lanes write neighbouring blocks. No LDS, no atomics
#include <algorithm>

#include "../backend.h"
#include "../device/bc_decode.h"
#include "../device/depth_prepass_raster.h"
#include "../device/texture_build.h"

namespace plr {
namespace texbuild {

struct ChainParams {
    const ChainJob* jobs;
    uint32_t* store;
    uint32_t* staging; // null: no job names it (the launcher checked)
    uint64_t storeWords, stagingWords;
    uint32_t firstJob, jobCount;
};

// the job of this workgroup: the last one of [first, first + count) whose firstGroup is not above `group`
template <class Job> PLR_DI uint32_t jobOfGroup(const Job* jobs, uint32_t first, uint32_t count, uint32_t group) {
    uint32_t lo = 0u, hi = count; // jobs[first + lo].firstGroup <= group < jobs[first + hi].firstGroup
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (jobs[first + mid].firstGroup <= group) lo = mid; else hi = mid;
    }
    return first + lo;
}

PLR_DI uint32_t wordAt(const uint32_t* words, uint64_t wordCount, uint64_t at) { return at < wordCount ? words[at] : 0u; }

__global__ void __launch_bounds__(kGroupLanes) textureMipChainKernel(ChainParams p) {
    const ChainJob job = p.jobs[jobOfGroup(p.jobs, p.firstJob, p.jobCount, blockIdx.x)];
    const uint32_t w = job.srcWidth, h = job.srcHeight;
    const uint32_t nw = w > 1u ? w >> 1 : 1u, nh = h > 1u ? h >> 1 : 1u;
    const uint32_t item = (blockIdx.x - job.firstGroup) * kGroupLanes + threadIdx.x;
    if (item >= nw * nh) return;
    const uint32_t y = item / nw, x = item - y * nw;
    const uint32_t x0 = min(2u * x, w - 1u), x1 = min(2u * x + 1u, w - 1u), y0 = min(2u * y, h - 1u), y1 = min(2u * y + 1u, h - 1u);
    const bool srcStaging = (job.flags & kChainSrcStaging) != 0u, dstStaging = (job.flags & kChainDstStaging) != 0u;
    const uint32_t* src = srcStaging ? p.staging : p.store;
    const uint64_t srcWords = srcStaging ? p.stagingWords : p.storeWords;
    const uint32_t format = job.flags & kChainFormatMask;
    uint32_t a, b, c, d;
    if (format == prepass::kTextureFormatRgba8) {
        const uint64_t r0 = (uint64_t)job.src + (uint64_t)y0 * w + x0, r1 = (uint64_t)job.src + (uint64_t)y1 * w + x0;
        if (x1 == x0 + 1u && (r0 & 1u) == 0u && r0 + 2u <= srcWords) { const uint2 v = *(const uint2*)(src + r0); a = v.x; b = v.y; }
        else { a = wordAt(src, srcWords, r0); b = wordAt(src, srcWords, r0 + (x1 - x0)); }
        if (x1 == x0 + 1u && (r1 & 1u) == 0u && r1 + 2u <= srcWords) { const uint2 v = *(const uint2*)(src + r1); c = v.x; d = v.y; }
        else { c = wordAt(src, srcWords, r1); d = wordAt(src, srcWords, r1 + (x1 - x0)); }
    } else if ((job.src & (prepass::blockWords(format) - 1u)) != 0u) {
        a = b = c = d = 0u; // blocks that are not at a multiple of their size: unusable, as in the prepass
    } else { // the level below is compressed: its texels through the block decode, which checks the block's address itself
        a = prepass::blockTexel<0>(src, srcWords, job.src, format, (int)w, (int)x0, (int)y0);
        b = prepass::blockTexel<0>(src, srcWords, job.src, format, (int)w, (int)x1, (int)y0);
        c = prepass::blockTexel<0>(src, srcWords, job.src, format, (int)w, (int)x0, (int)y1);
        d = prepass::blockTexel<0>(src, srcWords, job.src, format, (int)w, (int)x1, (int)y1);
    }
    const uint64_t at = (uint64_t)job.dst + item;
    if (at < (dstStaging ? p.stagingWords : p.storeWords)) (dstStaging ? p.staging : p.store)[at] = chainMean(a, b, c, d);
}

static int launchTextureMipChain(const PassCtx& c) {
    if (c.push.size() != sizeof(ChainPushConstants)) return c.fail(-1, "textureMipChain: push constants {firstJob, jobCount, groupCount, stagingBound} missing");
    ChainPushConstants pc{};
    std::memcpy(&pc, c.push.data(), sizeof(pc));
    if (pc.jobCount == 0u || pc.groupCount == 0u) return c.fail(-1, "textureMipChain: an execution without jobs or without workgroups");
    if (c.dispatch[0] != pc.groupCount || c.dispatch[1] != 1u || c.dispatch[2] != 1u || c.base[0] != 0u || c.base[1] != 0u)
        return c.fail(-1, "textureMipChain: the dispatch is {groupCount, 1, 1}: a lane per texel of the level built, the workgroups of a job from its firstGroup on");
    if (int rc = c.needSbuf(kChainJobBinding, ((size_t)pc.firstJob + pc.jobCount) * sizeof(ChainJob), "textureMipChain jobs (binding 0: {firstGroup, src, dst, srcWidth, srcHeight, flags, 0, 0} per job)")) return rc;
    if (int rc = c.needSbuf(kChainStoreBinding, 0, "textureMipChain texel store (binding 1)")) return rc;
    if (pc.stagingBound)
        if (int rc = c.needSbuf(kChainStagingBinding, 0, "textureMipChain staging chains (binding 2)")) return rc;
    if (c.sbuf[kChainStoreBinding].readOnly || (pc.stagingBound && c.sbuf[kChainStagingBinding].readOnly))
        return c.fail(-4, "textureMipChain: the texel store or the staging buffer (binding 1 or 2) is bound read-only");
    if (c.sbuf[kChainJobBinding].ptr == c.sbuf[kChainStoreBinding].ptr || (pc.stagingBound && c.sbuf[kChainJobBinding].ptr == c.sbuf[kChainStagingBinding].ptr))
        return c.fail(-4, "textureMipChain: an output buffer is also bound as the job table (binding 0)");
    if (pc.stagingBound && c.sbuf[kChainStoreBinding].ptr == c.sbuf[kChainStagingBinding].ptr) return c.fail(-4, "textureMipChain: the texel store and the staging buffer are one buffer");
    if (((uintptr_t)c.sbuf[kChainStoreBinding].ptr & 15u) != 0u || (pc.stagingBound && ((uintptr_t)c.sbuf[kChainStagingBinding].ptr & 15u) != 0u))
        return c.fail(-4, "textureMipChain: the texel store or the staging buffer (binding 1 or 2) is not at a 16-byte address");
    ChainParams p{};
    p.jobs = (const ChainJob*)c.sbuf[kChainJobBinding].ptr;
    p.store = (uint32_t*)c.sbuf[kChainStoreBinding].ptr; p.storeWords = c.sbuf[kChainStoreBinding].size / 4u;
    // without a staging buffer a job that names it reads zeros and writes nothing: the word count is 0
    p.staging = pc.stagingBound ? (uint32_t*)c.sbuf[kChainStagingBinding].ptr : nullptr; p.stagingWords = pc.stagingBound ? c.sbuf[kChainStagingBinding].size / 4u : 0u;
    p.firstJob = pc.firstJob; p.jobCount = pc.jobCount;
    textureMipChainKernel<<<pc.groupCount, kGroupLanes, 0, c.stream>>>(p);
    PLR_CHECK_LAUNCH(c);
    return 0;
}

// ---- "textureBlockEncode.comp"
struct EncodeParams {
    const EncodeJob* jobs;
    uint32_t* store;
    const uint32_t* staging;
    uint64_t storeWords, stagingWords;
    uint32_t jobCount;
};

__global__ void __launch_bounds__(kGroupLanes) textureBlockEncodeKernel(EncodeParams p) {
    const EncodeJob job = p.jobs[jobOfGroup(p.jobs, 0u, p.jobCount, blockIdx.x)];
    const uint32_t w = job.width, h = job.height, format = job.format;
    const uint32_t blocksX = (w + 3u) >> 2, blocksY = (h + 3u) >> 2;
    const uint32_t item = (blockIdx.x - job.firstGroup) * kGroupLanes + threadIdx.x;
    if (item >= blocksX * blocksY || format < prepass::kTextureFormatBc1 || format > prepass::kTextureFormatBc5 || w == 0u || h == 0u) return;
    const uint32_t by = item / blocksX, bx = item - by * blocksX;
    uint32_t t[16];
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t y = min(4u * by + j, h - 1u);
        const uint64_t row = (uint64_t)job.src + (uint64_t)y * w;
        const uint64_t at = row + 4u * bx;
        if (4u * bx + 3u < w && (at & 3u) == 0u && at + 4u <= p.stagingWords) {
            const uint4 v = *(const uint4*)(p.staging + at);
            t[4u * j] = v.x; t[4u * j + 1u] = v.y; t[4u * j + 2u] = v.z; t[4u * j + 3u] = v.w;
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) t[4u * j + i] = wordAt(p.staging, p.stagingWords, row + min(4u * bx + i, w - 1u));
        }
    }
    uint32_t out[4];
    encodeBlock(format, t, out);
    const uint32_t words = prepass::blockWords(format);
    const uint64_t at = (uint64_t)job.dst + (uint64_t)item * words;
    if ((at & (words - 1u)) != 0u || at + words > p.storeWords) return;
    if (words == 2u) *(uint2*)(p.store + at) = make_uint2(out[0], out[1]);
    else *(uint4*)(p.store + at) = make_uint4(out[0], out[1], out[2], out[3]);
}

static int launchTextureBlockEncode(const PassCtx& c) {
    if (c.push.size() != sizeof(EncodePushConstants)) return c.fail(-1, "textureBlockEncode: push constants {jobCount, groupCount} missing");
    EncodePushConstants pc{};
    std::memcpy(&pc, c.push.data(), sizeof(pc));
    if (pc.jobCount == 0u || pc.groupCount == 0u) return c.fail(-1, "textureBlockEncode: an execution without jobs or without workgroups");
    if (c.dispatch[0] != pc.groupCount || c.dispatch[1] != 1u || c.dispatch[2] != 1u || c.base[0] != 0u || c.base[1] != 0u)
        return c.fail(-1, "textureBlockEncode: the dispatch is {groupCount, 1, 1}: a lane per block, the workgroups of a job from its firstGroup on");
    if (int rc = c.needSbuf(kEncodeJobBinding, (size_t)pc.jobCount * sizeof(EncodeJob), "textureBlockEncode jobs (binding 0: {firstGroup, src, dst, width, height, format, 0, 0} per job)")) return rc;
    if (int rc = c.needSbuf(kEncodeStoreBinding, 0, "textureBlockEncode texel store (binding 1)")) return rc;
    if (int rc = c.needSbuf(kEncodeStagingBinding, 0, "textureBlockEncode staging chains (binding 2)")) return rc;
    if (c.sbuf[kEncodeStoreBinding].readOnly) return c.fail(-4, "textureBlockEncode: the texel store (binding 1) is bound read-only");
    for (int in : {kEncodeJobBinding, kEncodeStagingBinding})
        if (c.sbuf[in].ptr == c.sbuf[kEncodeStoreBinding].ptr) return c.fail(-4, "textureBlockEncode: the texel store is also bound as an input (binding " + std::to_string(in) + ")");
    if (((uintptr_t)c.sbuf[kEncodeStoreBinding].ptr & 15u) != 0u || ((uintptr_t)c.sbuf[kEncodeStagingBinding].ptr & 15u) != 0u)
        return c.fail(-4, "textureBlockEncode: the texel store or the staging buffer (binding 1 or 2) is not at a 16-byte address");
    EncodeParams p{};
    p.jobs = (const EncodeJob*)c.sbuf[kEncodeJobBinding].ptr;
    p.store = (uint32_t*)c.sbuf[kEncodeStoreBinding].ptr; p.storeWords = c.sbuf[kEncodeStoreBinding].size / 4u;
    p.staging = (const uint32_t*)c.sbuf[kEncodeStagingBinding].ptr; p.stagingWords = c.sbuf[kEncodeStagingBinding].size / 4u;
    p.jobCount = pc.jobCount;
    textureBlockEncodeKernel<<<pc.groupCount, kGroupLanes, 0, c.stream>>>(p);
    PLR_CHECK_LAUNCH(c);
    return 0;
}

} // namespace texbuild
static int texture_mip_chain_launch(const PassCtx& c) { return texbuild::launchTextureMipChain(c); }
static int texture_mip_chain_launch_fast(const PassCtx& c) { return texbuild::launchTextureMipChain(c); }
static int texture_block_encode_launch(const PassCtx& c) { return texbuild::launchTextureBlockEncode(c); }
static int texture_block_encode_launch_fast(const PassCtx& c) { return texbuild::launchTextureBlockEncode(c); }
PLR_REGISTER_SHADER("textureMipChain.comp", texture_mip_chain_launch);
PLR_REGISTER_SHADER_FAST("textureMipChain.comp", texture_mip_chain_launch_fast);
PLR_REGISTER_SHADER("textureBlockEncode.comp", texture_block_encode_launch);
PLR_REGISTER_SHADER_FAST("textureBlockEncode.comp", texture_block_encode_launch_fast);
} // namespace plr
