// Stand-alone check of the shadow caster cutout validation and packing (csrc/frontend/scene_packing.cpp) for a sanitizer run on the CPU; no GPU and no backend:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/shadow_cutout_check.cpp plainrenderer_amd/csrc/frontend/scene_packing.cpp -o shadow_cutout_check
//   ./shadow_cutout_check
// It packs textures (chains given and chains built), UVs and cutouts for caster sets of several sizes, compares every packed word with its source, and sends each
// kind of invalid input through the validation: every refusal must name its cause and none may read outside the caller's arrays (heap blocks of exactly the
// stated size, so the sanitizer sees an overrun).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../plainrenderer_amd/csrc/device/sun_shadow_raster.h"
#include "../plainrenderer_amd/csrc/frontend/frame_pipeline.h"

using namespace plrhost;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

static size_t chainTexels(uint32_t w, uint32_t h, uint32_t levels) {
    size_t n = 0;
    for (uint32_t l = 0; l < levels; l++) n += (size_t)std::max(1u, w >> l) * std::max(1u, h >> l);
    return n;
}

// a texture whose texels lie in a heap block of exactly the size its mip_count states (0: level 0 alone)
struct OwnedTexture {
    std::unique_ptr<uint32_t[]> texels;
    SceneTexture view;
    OwnedTexture(uint32_t w, uint32_t h, uint32_t mips, uint32_t salt) {
        const size_t n = chainTexels(w, h, std::max(1u, mips));
        texels.reset(new uint32_t[n]);
        for (size_t i = 0; i < n; i++) texels[i] = (uint32_t)(i * 2654435761u + salt);
        view = SceneTexture{texels.get(), w, h, mips};
    }
};

// the caster set of the checks: three meshes of 5, 0 and 7 vertices, four draws
static const uint32_t kVertexCounts[3] = {5u, 0u, 7u};
static const uint32_t kDraws = 4u;

struct Inputs {
    std::vector<OwnedTexture> owned;
    std::vector<SceneTexture> textures;
    std::unique_ptr<float[]> uv0, uv2;
    const float* uvs[3];
    std::unique_ptr<ShadowCutout[]> cutouts;
    Inputs() {
        owned.emplace_back(8u, 4u, 0u, 1u);  // the host builds the chain
        owned.emplace_back(5u, 3u, 3u, 2u);  // a full chain, given, not a power of two
        owned.emplace_back(16u, 16u, 2u, 3u); // two of five levels
        owned.emplace_back(1u, 1u, 1u, 4u);
        for (const OwnedTexture& t : owned) textures.push_back(t.view);
        uv0.reset(new float[10]); uv2.reset(new float[14]);
        for (int i = 0; i < 10; i++) uv0[i] = 0.125f * (float)i - 0.5f;
        for (int i = 0; i < 14; i++) uv2[i] = 3.f - 0.25f * (float)i;
        uvs[0] = uv0.get(); uvs[1] = nullptr; uvs[2] = uv2.get();
        cutouts.reset(new ShadowCutout[kDraws]);
        cutouts[0] = ShadowCutout{0u, 128u}; cutouts[1] = ShadowCutout{kNoSceneTexture, 0u}; cutouts[2] = ShadowCutout{3u, 255u}; cutouts[3] = ShadowCutout{1u, 1u};
    }
    PackedShadowCutouts pack(uint32_t textureCount = 4u, uint32_t meshCount = 3u, uint32_t drawCount = kDraws, uint32_t casterMeshes = 3u, uint32_t casterDraws = kDraws) const {
        return packShadowCasterCutouts(textures.data(), textureCount, uvs, meshCount, cutouts.get(), drawCount, kVertexCounts, casterMeshes, casterDraws);
    }
};

template <class F> static std::string refusal(F&& call, int* code) {
    try {
        call();
    } catch (const FramePipelineRefusal& e) {
        *code = e.code;
        return e.what();
    }
    *code = 0;
    return "";
}

int main() {
    static_assert(sizeof(plr::sunraster::CasterMaterial) == 8 && sizeof(plr::sunraster::CutoutPushConstants) == 12, "pass record");
    static_assert(plr::sunraster::kUvBinding == 6 && plr::sunraster::kCasterMaterialBinding == 7 && plr::sunraster::kTextureBinding == 8 && plr::sunraster::kTexelBinding == 9, "bindings");
    static_assert(plr::sunraster::scratchBytes(5) == 64 + 32 + 400 && plr::sunraster::cutoutScratchBytes(5) == 64 + 32 + 640, "scratch size formulas");
    static_assert(sizeof(ShadowCutout) == 8, "ShadowCutout layout");
    {
        const Inputs in;
        const PackedShadowCutouts p = in.pack();
        CHECK(p.tested && p.uvs.size() == 24 && p.materials.size() == 8 && p.textures.size() == 16);
        CHECK(std::memcmp(p.uvs.data(), in.uv0.get(), 40) == 0 && std::memcmp(p.uvs.data() + 10, in.uv2.get(), 56) == 0);
        for (uint32_t d = 0; d < kDraws; d++) CHECK(p.materials[2 * d] == in.cutouts[d].albedoTexture && p.materials[2 * d + 1] == in.cutouts[d].alphaCutoff);
        const uint32_t mips[4] = {4u, 3u, 2u, 1u};
        size_t at = 0;
        for (uint32_t t = 0; t < 4; t++) {
            const SceneTexture& s = in.textures[t];
            CHECK(p.textures[4 * t] == at && p.textures[4 * t + 1] == s.width && p.textures[4 * t + 2] == s.height && p.textures[4 * t + 3] == mips[t]);
            CHECK(std::memcmp(p.texels.data() + at, s.texels, chainTexels(s.width, s.height, std::max(1u, s.mipCount)) * 4u) == 0);
            at += chainTexels(s.width, s.height, mips[t]);
        }
        CHECK(p.texels.size() == at);
        // the built chain of texture 0: level 1 texel (0, 0), channel by channel, is the rounded mean of the 2 x 2 block
        uint32_t want = 0;
        for (int k = 0; k < 32; k += 8) {
            uint32_t sum = 2u;
            for (uint32_t i : {0u, 1u, 8u, 9u}) sum += (in.textures[0].texels[i] >> k) & 255u;
            want |= (sum >> 2) << k;
        }
        CHECK(p.texels[32] == want);
    }
    {
        Inputs in; // all cutoffs 0: the frames record the 8-byte push
        for (uint32_t d = 0; d < kDraws; d++) in.cutouts[d].alphaCutoff = 0u;
        CHECK(!in.pack().tested);
        in.cutouts[3].alphaCutoff = 1u;
        CHECK(in.pack().tested);
        const float* none[3] = {nullptr, nullptr, nullptr};
        const PackedShadowCutouts p = packShadowCasterCutouts(in.textures.data(), 4u, none, 3u, in.cutouts.get(), kDraws, kVertexCounts, 3u, kDraws);
        CHECK(p.uvs == std::vector<float>(24, 0.f)); // meshes given without UVs: (0, 0)
        CHECK(packShadowCasterCutouts(in.textures.data(), 4u, nullptr, 3u, in.cutouts.get(), kDraws, kVertexCounts, 3u, kDraws).uvs == p.uvs);
    }
    int code = 0;
    std::string why;
    auto has = [&](const char* word) { return why.find(word) != std::string::npos; };
    {
        const Inputs in;
        why = refusal([&] { in.pack(4u, 3u, kDraws, 0u, 0u); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("setShadowCasterCutouts") && has("no casters set"));
        why = refusal([&] { in.pack(4u, 2u); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mesh count 2") && has("mesh count 3"));
        why = refusal([&] { in.pack(4u, 3u, 3u); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("draw count 3") && has("draw count 4"));
        why = refusal([&] { packShadowCasterCutouts(nullptr, 4u, in.uvs, 3u, in.cutouts.get(), kDraws, kVertexCounts, 3u, kDraws); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null"));
        why = refusal([&] { packShadowCasterCutouts(in.textures.data(), 4u, in.uvs, 3u, nullptr, kDraws, kVertexCounts, 3u, kDraws); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null"));
        why = refusal([&] { in.pack(1u); }, &code); // draw 2 names texture 3 of 1
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("texture index out of range") && has("draw 2") && has("texture 3 of 1"));
    }
    for (uint32_t bad : {256u, 300u, 0xffffffffu}) {
        Inputs in;
        in.cutouts[1].alphaCutoff = bad;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("cutoff out of range") && has("draw 1") && has(std::to_string(bad).c_str()));
    }
    {
        Inputs in;
        in.textures[2].width = 0u;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("texture size out of range") && has("texture 2"));
        in.textures[2].width = 16385u;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("texture size out of range") && has("16385"));
        in.textures[2].width = 16u; in.textures[2].mipCount = 6u;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("too many mips") && has("texture 2"));
        in.textures[2].mipCount = 2u; in.textures[3].texels = nullptr;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null texels") && has("texture 3"));
    }
    {
        Inputs in; // more than 2^28 texels in all: refused before a texel is read (the blocks hold one level-0 texel each)
        std::unique_ptr<uint32_t[]> one(new uint32_t[1]());
        for (SceneTexture& t : in.textures) t = SceneTexture{one.get(), 16384u, 16384u, 0u};
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("too many texels"));
    }
    for (float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()}) {
        Inputs in;
        in.uv2[13] = bad;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("non-finite UV") && has("vertex 6 of mesh 2"));
    }
    std::printf(g_failures ? "shadow_cutout_check: %d check(s) failed\n" : "shadow_cutout_check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
