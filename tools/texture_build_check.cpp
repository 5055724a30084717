// Stand-alone check of the host side of the texture store the GPU builds (csrc/frontend/scene_packing.cpp packSceneTextureBuild, encodeBlockCompressedLevel), for a
// sanitizer run on the CPU; no GPU and no backend:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/texture_build_check.cpp plainrenderer_amd/csrc/frontend/scene_packing.cpp -o texture_build_check
//   ./texture_build_check
// It lays out a build of every accepted format pair at odd sizes (the caller's arrays are heap blocks of exactly the stated size, so the sanitizer sees an overrun),
// checks that every job of the two tables reads and writes inside the store and the staging buffer, then EXECUTES the job tables on the host - the chain rule and the
// encode contract of device/texture_build.h, launch by launch - and compares the finished store word for word with packSceneTexturesFormatted fed the levels the
// host makes with appendMipChain, decodeBlockCompressedLevel and encodeBlockCompressedLevel. Refusals must name their cause.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../plainrenderer_amd/csrc/device/depth_prepass_raster.h"
#include "../plainrenderer_amd/csrc/device/texture_build.h"
#include "../plainrenderer_amd/csrc/frontend/frame_pipeline.h"

using namespace plrhost;
namespace pp = plr::prepass;
namespace tb = plr::texbuild;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

static uint32_t code(uint32_t format) { return format == PLR_FORMAT_RGBA8 ? pp::kTextureFormatRgba8 : format == PLR_FORMAT_BC1 ? pp::kTextureFormatBc1 : format == PLR_FORMAT_BC3 ? pp::kTextureFormatBc3 : pp::kTextureFormatBc5; }
static uint32_t levelDim(uint32_t v, uint32_t l) { return std::max(1u, v >> l); }

struct Source { uint32_t width, height, mips, format, stored; std::unique_ptr<uint8_t[]> data; uint64_t bytes; };

static Source makeSource(uint32_t w, uint32_t h, uint32_t mips, uint32_t format, uint32_t stored, uint32_t salt) {
    Source s{w, h, mips, format, stored, nullptr, pp::textureWords(code(format), w, h, std::max(1u, mips)) * 4u};
    s.data.reset(new uint8_t[s.bytes]);
    for (uint64_t i = 0; i < s.bytes; i++) s.data[i] = (uint8_t)((i * 37u + salt * 101u + (i >> 3) * 13u + (i >> 7) * 5u) & 255u);
    return s;
}

// all levels of the source as the store is to hold them, made with the host's own functions
static std::vector<uint8_t> expectedLevels(const Source& s, uint32_t* levels) {
    const uint32_t full = pp::fullMipCount(s.width, s.height);
    *levels = s.mips ? s.mips : full;
    std::vector<uint32_t> rgba; // the RGBA8 levels that are encoded, or stored
    size_t firstBuilt = 0;     // bytes of the source that are kept verbatim in front
    std::vector<uint8_t> out;
    if (s.format == PLR_FORMAT_RGBA8) {
        rgba.resize(s.bytes / 4u);
        std::memcpy(rgba.data(), s.data.get(), s.bytes);
        if (s.mips == 0) appendMipChain(rgba, s.width, s.height);
    } else {
        out.assign(s.data.get(), s.data.get() + s.bytes);
        if (s.mips != 0) return out;
        rgba.resize((size_t)s.width * s.height);
        decodeBlockCompressedLevel(s.format, s.width, s.height, s.data.get(), s.bytes, rgba.data());
        appendMipChain(rgba, s.width, s.height);
        firstBuilt = 1;
    }
    size_t at = 0;
    for (uint32_t l = 0; l < *levels; l++) {
        const uint32_t w = levelDim(s.width, l), h = levelDim(s.height, l);
        if (l >= firstBuilt) {
            if (s.stored == PLR_FORMAT_RGBA8) out.insert(out.end(), (const uint8_t*)(rgba.data() + at), (const uint8_t*)(rgba.data() + at + (size_t)w * h));
            else {
                const uint64_t bytes = pp::textureWords(code(s.stored), w, h, 1) * 4u;
                std::vector<uint8_t> blocks(bytes);
                encodeBlockCompressedLevel(s.stored, w, h, rgba.data() + at, blocks.data(), bytes);
                out.insert(out.end(), blocks.begin(), blocks.end());
            }
        }
        at += (size_t)w * h;
    }
    return out;
}

static uint32_t wordAt(const std::vector<uint32_t>& v, uint64_t at) { return at < v.size() ? v[at] : 0u; }

int main() {
    const std::vector<uint32_t> vertexCounts = {4, 0, 3};
    const uint32_t sizes[][2] = {{1, 1}, {2, 2}, {3, 5}, {4, 4}, {5, 7}, {64, 32}, {130, 67}, {1, 300}};
    std::vector<Source> sources;
    uint32_t salt = 1;
    for (const auto& wh : sizes) {
        const uint32_t full = pp::fullMipCount(wh[0], wh[1]);
        for (uint32_t stored : {PLR_FORMAT_RGBA8, PLR_FORMAT_BC1, PLR_FORMAT_BC3, PLR_FORMAT_BC5}) {
            sources.push_back(makeSource(wh[0], wh[1], 0, PLR_FORMAT_RGBA8, stored, salt++));
            sources.push_back(makeSource(wh[0], wh[1], std::min(full, 2u), PLR_FORMAT_RGBA8, stored, salt++));
            if (stored != PLR_FORMAT_RGBA8) {
                sources.push_back(makeSource(wh[0], wh[1], 0, stored, stored, salt++));
                sources.push_back(makeSource(wh[0], wh[1], full, stored, stored, salt++));
            }
        }
    }
    std::vector<SceneTextureSource> given;
    for (const Source& s : sources) given.push_back({s.data.get(), s.bytes, s.width, s.height, s.mips, s.format, s.stored});
    const std::vector<SceneMaterial> materials = {{0, 1}, {kNoSceneTexture, 2}, {(uint32_t)sources.size() - 1u, kNoSceneTexture}};
    const std::vector<const float*> uvs = {nullptr, nullptr, nullptr};
    PackedTextureBuild b = packSceneTextureBuild(given.data(), (uint32_t)given.size(), uvs.data(), 3, materials.data(), 3, vertexCounts.data(), 3, 3);

    // every job inside its buffers; then the job tables, executed
    std::vector<uint32_t> store = b.texels, staging = b.staging;
    CHECK(b.chainLaunches.size() <= tb::kMaxChainLaunches && !b.chainLaunches.empty() && !b.encodeJobs.empty());
    const tb::ChainJob* chain = (const tb::ChainJob*)b.chainJobs.data();
    for (const PackedTextureBuild::ChainLaunch& launch : b.chainLaunches) {
        uint32_t groups = 0;
        for (uint32_t j = launch.firstJob; j < launch.firstJob + launch.jobCount; j++) {
            const tb::ChainJob& job = chain[j];
            const uint32_t w = job.srcWidth, h = job.srcHeight, nw = levelDim(w, 1), nh = levelDim(h, 1), format = job.flags & tb::kChainFormatMask;
            std::vector<uint32_t>& src = (job.flags & tb::kChainSrcStaging) ? staging : store;
            std::vector<uint32_t>& dst = (job.flags & tb::kChainDstStaging) ? staging : store;
            CHECK(job.firstGroup == groups);
            groups += (nw * nh + tb::kGroupLanes - 1u) / tb::kGroupLanes;
            CHECK((uint64_t)job.src + pp::textureWords(format, w, h, 1) <= src.size() && (uint64_t)job.dst + (uint64_t)nw * nh <= dst.size());
            std::vector<uint32_t> below((size_t)w * h);
            if (format == pp::kTextureFormatRgba8) for (size_t i = 0; i < below.size(); i++) below[i] = wordAt(src, job.src + i);
            else decodeBlockCompressedLevel(format == pp::kTextureFormatBc1 ? PLR_FORMAT_BC1 : format == pp::kTextureFormatBc3 ? PLR_FORMAT_BC3 : PLR_FORMAT_BC5, w, h, src.data() + job.src,
                                            pp::textureWords(format, w, h, 1) * 4u, below.data());
            for (uint32_t y = 0; y < nh; y++)
                for (uint32_t x = 0; x < nw; x++) {
                    const uint32_t x0 = std::min(2u * x, w - 1u), x1 = std::min(2u * x + 1u, w - 1u), y0 = std::min(2u * y, h - 1u), y1 = std::min(2u * y + 1u, h - 1u);
                    const uint64_t at = (uint64_t)job.dst + (uint64_t)y * nw + x;
                    if (at < dst.size()) dst[at] = tb::chainMean(below[(size_t)y0 * w + x0], below[(size_t)y0 * w + x1], below[(size_t)y1 * w + x0], below[(size_t)y1 * w + x1]);
                }
        }
        CHECK(groups == launch.groupCount);
    }
    const tb::EncodeJob* encode = (const tb::EncodeJob*)b.encodeJobs.data();
    uint32_t groups = 0;
    for (size_t j = 0; j < b.encodeJobs.size() * 4u / sizeof(tb::EncodeJob); j++) {
        const tb::EncodeJob& job = encode[j];
        const uint32_t bw = (job.width + 3u) / 4u, bh = (job.height + 3u) / 4u, words = pp::blockWords(job.format);
        CHECK(job.firstGroup == groups && (job.src & 3u) == 0u && (job.dst & (words - 1u)) == 0u);
        groups += (bw * bh + tb::kGroupLanes - 1u) / tb::kGroupLanes;
        CHECK((uint64_t)job.src + (uint64_t)job.width * job.height <= staging.size() && (uint64_t)job.dst + (uint64_t)bw * bh * words <= store.size());
        for (uint32_t by = 0; by < bh; by++)
            for (uint32_t bx = 0; bx < bw; bx++) {
                uint32_t t[16], out[4];
                for (uint32_t k = 0; k < 16u; k++) t[k] = wordAt(staging, (uint64_t)job.src + (uint64_t)std::min(4u * by + (k >> 2), job.height - 1u) * job.width + std::min(4u * bx + (k & 3u), job.width - 1u));
                tb::encodeBlock(job.format, t, out);
                for (uint32_t k = 0; k < words; k++) { const uint64_t at = (uint64_t)job.dst + ((uint64_t)by * bw + bx) * words + k; if (at < store.size()) store[at] = out[k]; }
            }
    }
    CHECK(groups == b.encodeGroups);

    // the same textures with all their levels through the formatted packer
    std::vector<std::vector<uint8_t>> levels(sources.size());
    std::vector<SceneTextureData> formatted;
    for (size_t t = 0; t < sources.size(); t++) {
        uint32_t count = 0;
        levels[t] = expectedLevels(sources[t], &count);
        formatted.push_back({levels[t].data(), levels[t].size(), sources[t].width, sources[t].height, count, sources[t].stored});
    }
    const PackedFormattedTextures want = packSceneTexturesFormatted(formatted.data(), (uint32_t)formatted.size(), uvs.data(), 3, materials.data(), 3, vertexCounts.data(), 3, 3);
    CHECK(want.textures == b.textures && want.formats == b.formats && want.compressed == b.compressed && want.materials == b.materials && want.uvs == b.uvs);
    CHECK(want.texels.size() == store.size());
    size_t differing = 0;
    for (size_t i = 0; i < std::min(want.texels.size(), store.size()); i++) differing += want.texels[i] != store[i];
    CHECK(differing == 0);
    std::printf("texture build check: %zu textures, %zu store words, %zu staging words, %zu chain launches, %zu words differ\n", sources.size(), store.size(), staging.size(),
                b.chainLaunches.size(), differing);

    // refusals
    auto refusal = [&](std::vector<SceneTextureSource> t) -> std::string {
        try { packSceneTextureBuild(t.data(), (uint32_t)t.size(), uvs.data(), 3, materials.data(), 3, vertexCounts.data(), 3, 3); } catch (const FramePipelineRefusal& e) { return e.what(); }
        return "";
    };
    auto with = [&](size_t k, auto&& change) { std::vector<SceneTextureSource> t = given; change(t[k]); return t; };
    CHECK(refusal(with(2, [](SceneTextureSource& s) { s.format = PLR_FORMAT_BC1; s.storeFormat = PLR_FORMAT_BC3; })).find("unsupported format pair: texture 2") != std::string::npos);
    CHECK(refusal(with(0, [](SceneTextureSource& s) { s.storeFormat = 1; })).find("store_format 1") != std::string::npos);
    CHECK(refusal(with(1, [](SceneTextureSource& s) { s.bytes += 4; })).find("bytes mismatch: texture 1") != std::string::npos);
    CHECK(refusal(with(3, [](SceneTextureSource& s) { s.data = nullptr; })).find("null texels: texture 3") != std::string::npos);
    {   // the staging limit: 16384 x 16384 to BC1 needs 2^28 * 4 / 3 staging words, while its store entry fits
        std::vector<SceneTextureSource> t = {{sources[0].data.get(), 16384ull * 16384ull * 4ull, 16384, 16384, 0, PLR_FORMAT_RGBA8, PLR_FORMAT_BC1}};
        const std::vector<SceneMaterial> m = {{0, 0}, {0, 0}, {0, 0}};
        std::string what;
        try { packSceneTextureBuild(t.data(), 1, uvs.data(), 3, m.data(), 3, vertexCounts.data(), 3, 3); } catch (const FramePipelineRefusal& e) { what = e.what(); }
        CHECK(what.find("too many staging texels") != std::string::npos);
    }
    std::printf(g_failures ? "texture build check: %d FAILED\n" : "texture build check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
