// Stand-alone check of the validation and packing of shadow caster cutouts whose textures carry a format (csrc/frontend/scene_packing.cpp,
// packShadowCasterCutoutsFormatted) for a sanitizer run on the CPU; no GPU and no backend:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/shadow_cutout_bc_check.cpp plainrenderer_amd/csrc/frontend/scene_packing.cpp -o shadow_cutout_bc_check
//   ./shadow_cutout_bc_check
// It packs a store that mixes RGBA8 (a chain given, a chain built), BC1, BC3 and BC5 entries of odd sizes for a caster set, compares every packed word with its
// source and the layout with the scene packer's for the same textures (one packer serves both), checks that an all-RGBA8 call packs what the unformatted call
// packs, and sends each kind of invalid input through the validation: every refusal must name its cause and none may read outside the caller's arrays (the
// arrays are heap blocks of exactly the stated size, so the sanitizer sees an overrun).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../plainrenderer_amd/csrc/device/sun_shadow_raster.h"
#include "../plainrenderer_amd/csrc/frontend/frame_pipeline.h"

using namespace plrhost;
namespace pp = plr::prepass;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

static uint32_t formatCode(uint32_t format) { return format == PLR_FORMAT_RGBA8 ? pp::kTextureFormatRgba8 : format == PLR_FORMAT_BC1 ? pp::kTextureFormatBc1 : format == PLR_FORMAT_BC3 ? pp::kTextureFormatBc3 : pp::kTextureFormatBc5; }
static uint64_t bytesOf(uint32_t format, uint32_t w, uint32_t h, uint32_t mips) { return pp::textureWords(formatCode(format), w, h, mips) * 4u; }

// a texture whose data lie in a heap block of exactly the size its levels hold (mip_count 0: level 0 alone)
struct OwnedTexture {
    std::unique_ptr<uint8_t[]> bytes;
    SceneTextureData view;
    OwnedTexture(uint32_t format, uint32_t w, uint32_t h, uint32_t mips, uint32_t salt) {
        const size_t n = (size_t)bytesOf(format, w, h, std::max(1u, mips));
        bytes.reset(new uint8_t[n]);
        for (size_t i = 0; i < n; i++) bytes[i] = (uint8_t)((i * 37u + salt * 101u + (i >> 3) * 13u) & 255u);
        view = SceneTextureData{bytes.get(), n, w, h, mips, format};
    }
};

// the caster set of the checks: three meshes of 5, 0 and 7 vertices, four draws
static const uint32_t kVertexCounts[3] = {5u, 0u, 7u};
static const uint32_t kDraws = 4u;

struct Inputs {
    std::vector<OwnedTexture> owned;
    std::vector<SceneTextureData> textures;
    std::unique_ptr<float[]> uv0, uv2;
    const float* uvs[3];
    std::unique_ptr<ShadowCutout[]> cutouts;
    Inputs() {
        owned.emplace_back((uint32_t)PLR_FORMAT_RGBA8, 5u, 3u, 3u, 1u); // 18 words: the next entry needs two words of padding
        owned.emplace_back((uint32_t)PLR_FORMAT_BC3, 5u, 7u, 3u, 2u);   // 2 x 2, 1 x 1, 1 x 1 blocks
        owned.emplace_back((uint32_t)PLR_FORMAT_BC1, 9u, 1u, 2u, 3u);   // 3 and 1 blocks of 8 bytes: 8 words
        owned.emplace_back((uint32_t)PLR_FORMAT_RGBA8, 8u, 4u, 0u, 4u); // the host builds the chain
        owned.emplace_back((uint32_t)PLR_FORMAT_BC5, 1u, 1u, 1u, 5u);
        for (const OwnedTexture& t : owned) textures.push_back(t.view);
        uv0.reset(new float[10]); uv2.reset(new float[14]);
        for (int i = 0; i < 10; i++) uv0[i] = 0.125f * (float)i - 0.5f;
        for (int i = 0; i < 14; i++) uv2[i] = 3.f - 0.25f * (float)i;
        uvs[0] = uv0.get(); uvs[1] = nullptr; uvs[2] = uv2.get();
        cutouts.reset(new ShadowCutout[kDraws]);
        cutouts[0] = ShadowCutout{1u, 128u}; cutouts[1] = ShadowCutout{kNoSceneTexture, 0u}; cutouts[2] = ShadowCutout{4u, 255u}; cutouts[3] = ShadowCutout{0u, 1u};
    }
    PackedFormattedShadowCutouts pack(uint32_t textureCount = 5u, uint32_t meshCount = 3u, uint32_t drawCount = kDraws, uint32_t casterMeshes = 3u, uint32_t casterDraws = kDraws) const {
        return packShadowCasterCutoutsFormatted(textures.data(), textureCount, uvs, meshCount, cutouts.get(), drawCount, kVertexCounts, casterMeshes, casterDraws);
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
    static_assert(sizeof(plr::sunraster::FormatPushConstants) == 16 && sizeof(plr::sunraster::CutoutPushConstants) == 12, "pass record");
    static_assert(plr::sunraster::kTextureFormatBinding == 14 && plr::sunraster::kTextureFormatBinding == pp::kTextureFormatBinding, "binding 14 is the prepass's number");
    static_assert(sizeof(plr::sunraster::CutoutRecord) == 128, "a format-aware execution's scratch is the tested size");
    {
        const Inputs in;
        const PackedFormattedShadowCutouts p = in.pack();
        CHECK(p.tested && p.compressed && p.uvs.size() == 24 && p.materials.size() == 8 && p.textures.size() == 20 && p.formats.size() == 5);
        CHECK(std::memcmp(p.uvs.data(), in.uv0.get(), 40) == 0 && std::memcmp(p.uvs.data() + 10, in.uv2.get(), 56) == 0);
        for (uint32_t d = 0; d < kDraws; d++) CHECK(p.materials[2 * d] == in.cutouts[d].albedoTexture && p.materials[2 * d + 1] == in.cutouts[d].alphaCutoff);
        const uint32_t offsets[5] = {0u, 20u, 44u, 52u, 96u}, mips[5] = {3u, 3u, 2u, 4u, 1u}; // 18 -> 20; + 24; + 8; 52 + 32 + 8 + 2 + 1 = 95 -> 96
        for (uint32_t t = 0; t < 5; t++) {
            const SceneTextureData& s = in.textures[t];
            CHECK(p.textures[4 * t] == offsets[t] && p.textures[4 * t + 1] == s.width && p.textures[4 * t + 2] == s.height && p.textures[4 * t + 3] == mips[t]);
            CHECK(p.formats[t] == formatCode(s.format));
            CHECK(p.texels.size() >= offsets[t] + s.bytes / 4u && std::memcmp(p.texels.data() + offsets[t], s.data, (size_t)s.bytes) == 0);
            if (formatCode(s.format) != pp::kTextureFormatRgba8) CHECK(offsets[t] % pp::blockWords(formatCode(s.format)) == 0u);
        }
        CHECK(p.texels.size() == 100 && p.texels[18] == 0u && p.texels[19] == 0u && p.texels[95] == 0u);
        // one packer: the scene's call lays the same textures out the same way
        const uint32_t sceneCounts[1] = {3u};
        const SceneMaterial material{kNoSceneTexture, kNoSceneTexture};
        const PackedFormattedTextures scene = packSceneTexturesFormatted(in.textures.data(), 5u, nullptr, 1u, &material, 1u, sceneCounts, 1u, 1u);
        CHECK(scene.textures == p.textures && scene.texels == p.texels && scene.formats == p.formats && scene.compressed);
    }
    {
        // an all-RGBA8 call packs what the unformatted call packs, chains built included, and is not `compressed`
        Inputs in;
        std::vector<SceneTextureData> rgba = {in.textures[0], in.textures[3]};
        std::vector<SceneTexture> plain = {SceneTexture{(const uint32_t*)nullptr, 5u, 3u, 3u}, SceneTexture{(const uint32_t*)nullptr, 8u, 4u, 0u}};
        std::vector<uint32_t> words0(18), words3(32); // (aligned copies for the unformatted call's uint32 pointers)
        std::memcpy(words0.data(), in.textures[0].data, 72); std::memcpy(words3.data(), in.textures[3].data, 128);
        plain[0].texels = words0.data(); plain[1].texels = words3.data();
        in.cutouts[0].albedoTexture = 1u; in.cutouts[2].albedoTexture = 0u;
        const PackedFormattedShadowCutouts f = packShadowCasterCutoutsFormatted(rgba.data(), 2u, in.uvs, 3u, in.cutouts.get(), kDraws, kVertexCounts, 3u, kDraws);
        const PackedShadowCutouts u = packShadowCasterCutouts(plain.data(), 2u, in.uvs, 3u, in.cutouts.get(), kDraws, kVertexCounts, 3u, kDraws);
        CHECK(!f.compressed && f.tested == u.tested && f.textures == u.textures && f.texels == u.texels && f.materials == u.materials && f.uvs == u.uvs);
        CHECK(f.formats == std::vector<uint32_t>(2, pp::kTextureFormatRgba8));
        for (uint32_t d = 0; d < kDraws; d++) in.cutouts[d].alphaCutoff = 0u; // all cutoffs 0: the frames record the 8-byte push
        CHECK(!packShadowCasterCutoutsFormatted(rgba.data(), 2u, in.uvs, 3u, in.cutouts.get(), kDraws, kVertexCounts, 3u, kDraws).tested);
    }
    int code = 0;
    std::string why;
    auto has = [&](const char* word) { return why.find(word) != std::string::npos; };
    {
        // everything the unformatted call refuses
        const Inputs in;
        why = refusal([&] { in.pack(5u, 3u, kDraws, 0u, 0u); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("setShadowCasterCutoutsFormatted") && has("no casters set"));
        why = refusal([&] { in.pack(5u, 2u); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mesh count 2") && has("mesh count 3"));
        why = refusal([&] { in.pack(5u, 3u, 3u); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("draw count 3") && has("draw count 4"));
        why = refusal([&] { packShadowCasterCutoutsFormatted(nullptr, 5u, in.uvs, 3u, in.cutouts.get(), kDraws, kVertexCounts, 3u, kDraws); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null"));
        why = refusal([&] { packShadowCasterCutoutsFormatted(in.textures.data(), 5u, in.uvs, 3u, nullptr, kDraws, kVertexCounts, 3u, kDraws); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null"));
        why = refusal([&] { in.pack(2u); }, &code); // draw 2 names texture 4 of 2
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("texture index out of range") && has("draw 2") && has("texture 4 of 2"));
    }
    for (uint32_t bad : {256u, 300u, 0xffffffffu}) {
        Inputs in;
        in.cutouts[1].alphaCutoff = bad;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("cutoff out of range") && has("draw 1") && has(std::to_string(bad).c_str()));
    }
    {
        Inputs in;
        in.textures[1].width = 0u;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("texture size out of range") && has("texture 1"));
        in.textures[1].width = 16385u;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("texture size out of range") && has("16385"));
        in.textures[1].width = 5u; in.textures[1].mipCount = 4u;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("too many mips") && has("texture 1"));
        in.textures[1].mipCount = 3u; in.textures[4].data = nullptr;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null texels") && has("texture 4"));
    }
    {
        // what the format adds
        Inputs in;
        in.textures[2].format = 77u;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("unknown format") && has("texture 2") && has("77"));
        in.textures[2].format = PLR_FORMAT_BC1; in.textures[2].mipCount = 0u;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mip_count 0 on a compressed texture") && has("texture 2"));
        in.textures[2].mipCount = 2u;
        for (uint64_t off : {(uint64_t)31u, (uint64_t)33u, (uint64_t)0u}) { // (refused before a byte is read)
            in.textures[2].bytes = off;
            why = refusal([&] { in.pack(); }, &code);
            CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("bytes mismatch") && has("texture 2") && has("hold 32"));
        }
        in.textures[2].bytes = 32u;
        in.textures[0].bytes = 60u; // an RGBA8 entry: level 0 alone where three levels are stated
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("bytes mismatch") && has("texture 0") && has("hold 72"));
    }
    {
        Inputs in; // more than 2^28 words in all: refused before a block is read (the entries keep their small heap blocks)
        for (SceneTextureData& t : in.textures) { t.format = PLR_FORMAT_BC3; t.width = t.height = 16384u; t.mipCount = 1u; t.bytes = bytesOf(PLR_FORMAT_BC3, 16384u, 16384u, 1u); }
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("too many texels") && has("words"));
    }
    for (float bad : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()}) {
        Inputs in;
        in.uv2[13] = bad;
        why = refusal([&] { in.pack(); }, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("non-finite UV") && has("vertex 6 of mesh 2"));
    }
    std::printf(g_failures ? "shadow_cutout_bc_check: %d check(s) failed\n" : "shadow_cutout_bc_check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
