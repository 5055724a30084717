// Stand-alone check of the scene texture validation, packing and mip builder (csrc/frontend/scene_packing.cpp) for a sanitizer run on the CPU; no GPU and no
// backend:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/scene_texture_check.cpp plainrenderer_amd/csrc/frontend/scene_packing.cpp -o scene_texture_check
//   ./scene_texture_check
// It packs textures with caller-supplied and host-built chains, odd sizes included, compares every packed element with its source and every built level with the
// rule worked out here, and sends each kind of invalid input through the validation: every refusal must name its cause and none may read outside the caller's
// arrays (the arrays are heap blocks of exactly the stated size, so the sanitizer sees an overrun).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../plainrenderer_amd/csrc/device/depth_prepass_raster.h"
#include "../plainrenderer_amd/csrc/frontend/frame_pipeline.h"

using namespace plrhost;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

static uint32_t texel(uint32_t x, uint32_t y, uint32_t salt) { return ((x * 53u + y * 19u + salt) & 255u) | (((x * 11u + y * 97u) & 255u) << 8) | (((x * 151u + salt) & 255u) << 16) | (((y * 61u) & 255u) << 24); }

// `texels` texels in a heap block of exactly that size
static std::unique_ptr<uint32_t[]> block(uint32_t width, uint32_t height, uint32_t levels, uint32_t salt, size_t* count) {
    size_t n = 0;
    for (uint32_t l = 0; l < levels; l++) n += (size_t)std::max(1u, width >> l) * std::max(1u, height >> l);
    std::unique_ptr<uint32_t[]> b(new uint32_t[n]);
    size_t at = 0;
    for (uint32_t l = 0; l < levels; l++)
        for (uint32_t y = 0; y < std::max(1u, height >> l); y++)
            for (uint32_t x = 0; x < std::max(1u, width >> l); x++) b[at++] = texel(x, y, salt + 7u * l);
    *count = n;
    return b;
}

struct Scene {
    std::vector<uint32_t> vertexCounts = {4, 0, 3};
    uint32_t drawCount = 3;
};

static std::string refusal(const Scene& s, const std::vector<SceneTexture>& t, const std::vector<const float*>& uvs, const std::vector<SceneMaterial>& m, int* code) {
    try {
        packSceneTextures(t.data(), (uint32_t)t.size(), uvs.empty() ? nullptr : uvs.data(), (uint32_t)uvs.size(), m.data(), (uint32_t)m.size(), s.vertexCounts.data(),
                          (uint32_t)s.vertexCounts.size(), s.drawCount);
    } catch (const FramePipelineRefusal& e) {
        *code = e.code;
        return e.what();
    }
    *code = 0;
    return "";
}

int main() {
    const Scene scene;
    size_t n0, n1, n2, n3;
    std::unique_ptr<uint32_t[]> t0 = block(5, 3, 1, 1, &n0), t1 = block(8, 4, 4, 2, &n1), t2 = block(1, 1, 1, 3, &n2), t3 = block(16, 1, 1, 4, &n3);
    std::unique_ptr<float[]> uv0(new float[8]), uv2(new float[6]);
    for (int i = 0; i < 8; i++) uv0[i] = 0.25f * (float)i;
    for (int i = 0; i < 6; i++) uv2[i] = -1.5f * (float)i;
    const std::vector<SceneTexture> textures = {{t0.get(), 5, 3, 0}, {t1.get(), 8, 4, 4}, {t2.get(), 1, 1, 0}, {t3.get(), 16, 1, 0}};
    const std::vector<const float*> uvs = {uv0.get(), nullptr, uv2.get()};
    const std::vector<SceneMaterial> materials = {{0, kNoSceneTexture}, {kNoSceneTexture, kNoSceneTexture}, {3, 1}};
    const PackedTextures p = packSceneTextures(textures.data(), 4, uvs.data(), 3, materials.data(), 3, scene.vertexCounts.data(), 3, scene.drawCount);
    // UVs back to back in the order of the meshes, zeros for a mesh without
    CHECK(p.uvs.size() == 14 && std::memcmp(p.uvs.data(), uv0.get(), 32) == 0 && std::memcmp(p.uvs.data() + 8, uv2.get(), 24) == 0);
    CHECK(p.materials == std::vector<uint32_t>({0u, kNoSceneTexture, kNoSceneTexture, kNoSceneTexture, 3u, 1u}));
    plr::prepass::Texture e[4];
    std::memcpy(e, p.textures.data(), sizeof(e));
    // 5 x 3 -> 2 x 1 -> 1 x 1 (3 levels, 18 texels); 8 x 4 with its 4 levels (32 + 8 + 2 + 1 = 43); 1 x 1; 16 x 1 -> 8, 4, 2, 1 (31)
    CHECK(e[0].texelOffset == 0 && e[0].width == 5 && e[0].height == 3 && e[0].mipCount == 3);
    CHECK(e[1].texelOffset == 18 && e[1].mipCount == 4 && e[2].texelOffset == 61 && e[2].mipCount == 1 && e[3].texelOffset == 62 && e[3].mipCount == 5);
    CHECK(p.texels.size() == 18 + 43 + 1 + 31);
    CHECK(std::memcmp(p.texels.data(), t0.get(), 15 * 4) == 0 && std::memcmp(p.texels.data() + 18, t1.get(), 43 * 4) == 0 && p.texels[61] == t2[0]);
    // the built levels of the 5 x 3 texture by the rule: level 1 (2 x 1) texel x from columns 2x, 2x + 1 and rows 0, 1; level 2 from level 1's two texels twice
    for (uint32_t x = 0; x < 2; x++)
        for (int k = 0; k < 32; k += 8) {
            const uint32_t sum = ((t0[2 * x] >> k) & 255u) + ((t0[2 * x + 1] >> k) & 255u) + ((t0[5 + 2 * x] >> k) & 255u) + ((t0[5 + 2 * x + 1] >> k) & 255u);
            CHECK(((p.texels[15 + x] >> k) & 255u) == (sum + 2u) >> 2);
        }
    for (int k = 0; k < 32; k += 8) {
        const uint32_t a = (p.texels[15] >> k) & 255u, b = (p.texels[16] >> k) & 255u;
        CHECK(((p.texels[17] >> k) & 255u) == (a + b + a + b + 2u) >> 2); // H_l = 1: both rows are row 0
    }
    // 16 x 1: every level halves the row
    for (uint32_t x = 0; x < 8; x++) CHECK((p.texels[62 + 16 + x] & 255u) == ((t3[2 * x] & 255u) * 2u + (t3[2 * x + 1] & 255u) * 2u + 2u) >> 2);
    {
        std::vector<uint32_t> chain(t3.get(), t3.get() + 16);
        appendMipChain(chain, 16, 1);
        CHECK(chain.size() == 31 && std::memcmp(chain.data(), p.texels.data() + 62, 31 * 4) == 0);
        std::vector<uint32_t> one(1, 0x12345678u);
        appendMipChain(one, 1, 1);
        CHECK(one.size() == 1);
    }
    CHECK(plr::prepass::fullMipCount(1, 1) == 1 && plr::prepass::fullMipCount(5, 3) == 3 && plr::prepass::fullMipCount(16384, 1) == 15 && plr::prepass::fullMipCount(3, 64) == 7);

    int code = 0;
    std::string why;
    auto has = [&](const char* word) { return why.find(word) != std::string::npos; };
    Scene none;
    none.vertexCounts.clear(); none.drawCount = 0;
    why = refusal(none, textures, {}, {}, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("no scene set"));
    why = refusal(scene, textures, {uv0.get(), nullptr}, materials, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mesh count 2") && has("mesh count 3"));
    why = refusal(scene, textures, uvs, {materials[0], materials[1]}, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("draw count 2") && has("draw count 3"));
    for (uint32_t bad : {0u, 16385u}) {
        std::vector<SceneTexture> t = textures;
        t[1].width = bad;
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("texture size out of range") && has("texture 1"));
        t = textures;
        t[2].height = bad;
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("texture size out of range") && has("texture 2"));
    }
    {
        std::vector<SceneTexture> t = textures;
        t[1].mipCount = 5; // 8 x 4 has 4
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("too many mips") && has("texture 1") && has("at most 4"));
        t = textures;
        t[3].texels = nullptr;
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null texels") && has("texture 3"));
    }
    {
        std::vector<SceneMaterial> m = materials;
        m[2].specularTexture = 4;
        why = refusal(scene, textures, uvs, m, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("material texture index out of range") && has("draw 2") && has("texture 4 of 4"));
        m = materials;
        m[0].albedoTexture = 0xfffffffeu;
        why = refusal(scene, textures, uvs, m, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("draw 0"));
    }
    {
        // 2^28 texels are accepted in principle, one more is not: sizes are validated before anything is read, so a one-texel block stands in for the data
        std::vector<SceneTexture> t = {{t2.get(), 16384, 16384, 1}, {t2.get(), 1, 1, 1}};
        std::vector<SceneMaterial> m = {{0, 1}, {0, 1}, {0, 1}};
        why = refusal(scene, t, uvs, m, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("too many texels") && has("268435457"));
    }
    for (float v : {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()}) {
        uv2[5] = v;
        why = refusal(scene, textures, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("non-finite UV") && has("vertex 2 of mesh 2"));
        uv2[5] = -7.5f;
    }
    why = refusal(scene, textures, uvs, materials, &code);
    CHECK(code == 0);
    why = refusal(scene, textures, {}, materials, &code); // a null UV array needs a matching mesh count all the same
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mesh count 0"));
    std::printf(g_failures ? "scene_texture_check: %d check(s) failed\n" : "scene_texture_check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
