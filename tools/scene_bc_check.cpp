// Stand-alone check of the validation and packing of scene textures that carry a format, and of the host's BC1 / BC3 / BC5 decoder (csrc/frontend/scene_packing.cpp),
// for a sanitizer run on the CPU; no GPU and no backend:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/scene_bc_check.cpp plainrenderer_amd/csrc/frontend/scene_packing.cpp -o scene_bc_check
//   ./scene_bc_check
// It packs a store that mixes the four formats, odd sizes included (1 x 1, 5 x 7, 16384 x 1), and compares every packed word with its source; decodes levels of
// those sizes and compares blocks worked out here by hand; and sends each kind of invalid input through the validation: every refusal must name its cause and
// none may read outside the caller's arrays (the arrays are heap blocks of exactly the stated size, so the sanitizer sees an overrun).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../plainrenderer_amd/csrc/device/depth_prepass_raster.h"
#include "../plainrenderer_amd/csrc/frontend/frame_pipeline.h"

using namespace plrhost;
namespace pp = plr::prepass;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

// `bytes` bytes in a heap block of exactly that size
static std::unique_ptr<uint8_t[]> block(size_t bytes, uint32_t salt) {
    std::unique_ptr<uint8_t[]> b(new uint8_t[bytes]);
    for (size_t i = 0; i < bytes; i++) b[i] = (uint8_t)((i * 37u + salt * 101u + (i >> 3) * 13u) & 255u);
    return b;
}
static uint32_t formatCode(uint32_t format) { return format == PLR_FORMAT_RGBA8 ? pp::kTextureFormatRgba8 : format == PLR_FORMAT_BC1 ? pp::kTextureFormatBc1 : format == PLR_FORMAT_BC3 ? pp::kTextureFormatBc3 : pp::kTextureFormatBc5; }
static uint64_t bytesOf(uint32_t format, uint32_t w, uint32_t h, uint32_t mips) { return pp::textureWords(formatCode(format), w, h, mips) * 4u; }

struct Scene {
    std::vector<uint32_t> vertexCounts = {4, 0, 3};
    uint32_t drawCount = 3;
};

static std::string refusal(const Scene& s, const std::vector<SceneTextureData>& t, const std::vector<const float*>& uvs, const std::vector<SceneMaterial>& m, int* code) {
    try {
        packSceneTexturesFormatted(t.data(), (uint32_t)t.size(), uvs.empty() ? nullptr : uvs.data(), (uint32_t)uvs.size(), m.data(), (uint32_t)m.size(), s.vertexCounts.data(),
                                   (uint32_t)s.vertexCounts.size(), s.drawCount);
    } catch (const FramePipelineRefusal& e) {
        *code = e.code;
        return e.what();
    }
    *code = 0;
    return "";
}
static std::string decodeRefusal(uint32_t format, uint32_t w, uint32_t h, const void* blocks, uint64_t bytes, uint32_t* out, int* code) {
    try {
        decodeBlockCompressedLevel(format, w, h, blocks, bytes, out);
    } catch (const FramePipelineRefusal& e) {
        *code = e.code;
        return e.what();
    }
    *code = 0;
    return "";
}

static void checkDecoder() {
    // one colour block by hand: c0 = (25, 50, 4) -> (206, 203, 33), c1 = (3, 9, 30) -> (24, 36, 247); indices 0, 1, 2, 3 repeated
    const uint16_t hi = (25u << 11) | (50u << 5) | 4u, lo = (3u << 11) | (9u << 5) | 30u;
    auto colour = [](uint16_t c0, uint16_t c1, uint8_t* b) {
        b[0] = (uint8_t)(c0 & 255u); b[1] = (uint8_t)(c0 >> 8); b[2] = (uint8_t)(c1 & 255u); b[3] = (uint8_t)(c1 >> 8);
        b[4] = b[5] = b[6] = b[7] = 0xE4; // 3 2 1 0 per byte, texel i at bits 2 i
    };
    auto alpha = [](uint8_t a0, uint8_t a1, uint8_t* b) { // indices 0 .. 7 twice: 24 bits 0xFAC688 twice
        b[0] = a0; b[1] = a1;
        const uint64_t bits = 0xFAC688ull | (0xFAC688ull << 24);
        for (int k = 0; k < 6; k++) b[2 + k] = (uint8_t)((bits >> (8 * k)) & 255u);
    };
    auto word = [](uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return r | (g << 8) | (b << 16) | (a << 24); };
    std::unique_ptr<uint8_t[]> bc1(new uint8_t[8]), bc3(new uint8_t[16]), bc5(new uint8_t[16]);
    std::unique_ptr<uint32_t[]> out(new uint32_t[16]);
    colour(hi, lo, bc1.get());
    decodeBlockCompressedLevel(PLR_FORMAT_BC1, 4, 4, bc1.get(), 8, out.get());
    CHECK(out[0] == word(206, 203, 33, 255) && out[1] == word(24, 36, 247, 255) && out[2] == word(145, 147, 104, 255) && out[3] == word(85, 92, 176, 255) && out[15] == out[3]);
    colour(lo, hi, bc1.get()); // three-colour mode: the mean and opaque black
    decodeBlockCompressedLevel(PLR_FORMAT_BC1, 4, 4, bc1.get(), 8, out.get());
    CHECK(out[0] == word(24, 36, 247, 255) && out[1] == word(206, 203, 33, 255) && out[2] == word(115, 120, 140, 255) && out[3] == word(0, 0, 0, 255));
    colour(hi, hi, bc1.get());
    decodeBlockCompressedLevel(PLR_FORMAT_BC1, 4, 4, bc1.get(), 8, out.get());
    CHECK(out[2] == word(206, 203, 33, 255) && out[3] == word(0, 0, 0, 255));
    alpha(200, 31, bc3.get());
    colour(lo, hi, bc3.get() + 8); // BC3: four-colour mode although c0 <= c1
    decodeBlockCompressedLevel(PLR_FORMAT_BC3, 4, 4, bc3.get(), 16, out.get());
    const uint32_t eight[8] = {200, 31, 176, 152, 128, 103, 79, 55}, six[8] = {31, 200, 65, 99, 132, 166, 0, 255};
    CHECK(out[2] == word(85, 92, 176, 176) && out[3] == word(145, 147, 104, 152) && out[0] == word(24, 36, 247, 200));
    for (int i = 0; i < 16; i++) CHECK((out[i] >> 24) == eight[i & 7]);
    alpha(31, 200, bc5.get());
    alpha(200, 31, bc5.get() + 8);
    decodeBlockCompressedLevel(PLR_FORMAT_BC5, 4, 4, bc5.get(), 16, out.get());
    for (int i = 0; i < 16; i++) CHECK(out[i] == word(six[i & 7], eight[i & 7], 0, 255));
    // odd sizes: 1 x 1 is position 0 of its block; 5 x 7 is 2 x 2 blocks; 16384 x 1 is 4096 blocks of which row 0 alone is addressed
    std::unique_ptr<uint32_t[]> one(new uint32_t[1]);
    decodeBlockCompressedLevel(PLR_FORMAT_BC5, 1, 1, bc5.get(), 16, one.get());
    CHECK(one[0] == word(31, 200, 0, 255));
    {
        std::unique_ptr<uint8_t[]> blocks = block(64, 3);
        std::unique_ptr<uint32_t[]> level(new uint32_t[35]), single(new uint32_t[16]);
        decodeBlockCompressedLevel(PLR_FORMAT_BC3, 5, 7, blocks.get(), 64, level.get());
        for (uint32_t b = 0; b < 4; b++) {
            decodeBlockCompressedLevel(PLR_FORMAT_BC3, 4, 4, blocks.get() + 16 * b, 16, single.get());
            for (uint32_t y = 0; y < 4; y++)
                for (uint32_t x = 0; x < 4; x++) {
                    const uint32_t X = 4 * (b & 1) + x, Y = 4 * (b >> 1) + y;
                    if (X < 5 && Y < 7) CHECK(level[Y * 5 + X] == single[4 * y + x]);
                }
        }
    }
    {
        const size_t bytes = 4096 * 8;
        std::unique_ptr<uint8_t[]> blocks = block(bytes, 4);
        std::unique_ptr<uint32_t[]> row(new uint32_t[16384]), single(new uint32_t[16]);
        decodeBlockCompressedLevel(PLR_FORMAT_BC1, 16384, 1, blocks.get(), bytes, row.get());
        for (uint32_t b : {0u, 1u, 2047u, 4095u}) {
            decodeBlockCompressedLevel(PLR_FORMAT_BC1, 4, 4, blocks.get() + 8 * b, 8, single.get());
            for (uint32_t x = 0; x < 4; x++) CHECK(row[4 * b + x] == single[x]);
        }
    }
    int code = 0;
    std::string why;
    auto has = [&](const char* w) { return why.find(w) != std::string::npos; };
    why = decodeRefusal(PLR_FORMAT_RGBA8, 4, 4, bc1.get(), 8, out.get(), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("format 2") && has("PLR_FORMAT_BC1"));
    why = decodeRefusal(99, 4, 4, bc1.get(), 8, out.get(), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("format 99"));
    why = decodeRefusal(PLR_FORMAT_BC1, 0, 4, bc1.get(), 8, out.get(), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("0 x 4"));
    why = decodeRefusal(PLR_FORMAT_BC1, 4, 16385, bc1.get(), 8, out.get(), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("16385"));
    why = decodeRefusal(PLR_FORMAT_BC1, 4, 4, nullptr, 8, out.get(), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null"));
    why = decodeRefusal(PLR_FORMAT_BC1, 4, 4, bc1.get(), 8, nullptr, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null"));
    why = decodeRefusal(PLR_FORMAT_BC1, 5, 4, bc1.get(), 8, out.get(), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("bytes mismatch") && has("holds 16"));
    why = decodeRefusal(PLR_FORMAT_BC3, 4, 4, bc3.get(), 8, out.get(), &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("bytes mismatch"));
}

int main() {
    checkDecoder();
    const Scene scene;
    // RGBA8 5 x 3 with a host-built chain (15 texels given, 18 packed); BC1 5 x 7 with 3 levels (2 x 2, 1, 1 blocks: 48 bytes); RGBA8 1 x 1; BC3 16384 x 1 with 2
    // levels (4096 + 2048 blocks); BC5 1 x 1
    const uint64_t n0 = 15 * 4, n1 = bytesOf(PLR_FORMAT_BC1, 5, 7, 3), n2 = 4, n3 = bytesOf(PLR_FORMAT_BC3, 16384, 1, 2), n4 = bytesOf(PLR_FORMAT_BC5, 1, 1, 1);
    CHECK(n1 == 48 && n3 == (4096 + 2048) * 16 && n4 == 16);
    std::unique_ptr<uint8_t[]> t0 = block(n0, 1), t1 = block(n1, 2), t2 = block(n2, 3), t3 = block(n3, 4), t4 = block(n4, 5);
    std::unique_ptr<float[]> uv0(new float[8]), uv2(new float[6]);
    for (int i = 0; i < 8; i++) uv0[i] = 0.25f * (float)i;
    for (int i = 0; i < 6; i++) uv2[i] = -1.5f * (float)i;
    const std::vector<SceneTextureData> textures = {{t0.get(), n0, 5, 3, 0, PLR_FORMAT_RGBA8}, {t1.get(), n1, 5, 7, 3, PLR_FORMAT_BC1}, {t2.get(), n2, 1, 1, 1, PLR_FORMAT_RGBA8},
                                                    {t3.get(), n3, 16384, 1, 2, PLR_FORMAT_BC3}, {t4.get(), n4, 1, 1, 1, PLR_FORMAT_BC5}};
    const std::vector<const float*> uvs = {uv0.get(), nullptr, uv2.get()};
    const std::vector<SceneMaterial> materials = {{0, kNoSceneTexture}, {kNoSceneTexture, 4}, {3, 1}};
    const PackedFormattedTextures p = packSceneTexturesFormatted(textures.data(), 5, uvs.data(), 3, materials.data(), 3, scene.vertexCounts.data(), 3, scene.drawCount);
    CHECK(p.compressed && p.formats == std::vector<uint32_t>({pp::kTextureFormatRgba8, pp::kTextureFormatBc1, pp::kTextureFormatRgba8, pp::kTextureFormatBc3, pp::kTextureFormatBc5}));
    CHECK(p.uvs.size() == 14 && std::memcmp(p.uvs.data(), uv0.get(), 32) == 0 && std::memcmp(p.uvs.data() + 8, uv2.get(), 24) == 0);
    CHECK(p.materials == std::vector<uint32_t>({0u, kNoSceneTexture, kNoSceneTexture, 4u, 3u, 1u}));
    pp::Texture e[5];
    std::memcpy(e, p.textures.data(), sizeof(e));
    // 18 words -> the BC1 at 20 (12 words) -> RGBA8 at 32 -> the BC3 at 36 (24576 words) -> the BC5 at 24612 (4 words)
    CHECK(e[0].texelOffset == 0 && e[0].mipCount == 3 && e[1].texelOffset == 20 && e[1].mipCount == 3 && e[2].texelOffset == 32 && e[3].texelOffset == 36 && e[3].mipCount == 2 &&
          e[4].texelOffset == 24612);
    CHECK(p.texels.size() == 24616);
    CHECK(std::memcmp(p.texels.data(), t0.get(), n0) == 0 && std::memcmp(p.texels.data() + 20, t1.get(), n1) == 0 && std::memcmp(p.texels.data() + 32, t2.get(), n2) == 0 &&
          std::memcmp(p.texels.data() + 36, t3.get(), n3) == 0 && std::memcmp(p.texels.data() + 24612, t4.get(), n4) == 0);
    CHECK(p.texels[18] == 0 && p.texels[19] == 0 && p.texels[33] == 0 && p.texels[34] == 0 && p.texels[35] == 0); // the padding
    for (uint32_t t = 0; t < 5; t++) CHECK(p.formats[t] == pp::kTextureFormatRgba8 || e[t].texelOffset % 4u == 0u);
    {
        // the built levels of the RGBA8 5 x 3 texture are packSceneTextures' own
        const SceneTexture plain{(const uint32_t*)t0.get(), 5, 3, 0};
        const SceneMaterial m[3] = {{0, 0}, {0, 0}, {0, 0}};
        const PackedTextures q = packSceneTextures(&plain, 1, uvs.data(), 3, m, 3, scene.vertexCounts.data(), 3, scene.drawCount);
        CHECK(q.texels.size() == 18 && std::memcmp(q.texels.data(), p.texels.data(), 72) == 0);
        // ... and a call whose entries are all RGBA8 packs what packSceneTextures packs, and is not compressed
        const SceneTextureData same{t0.get(), n0, 5, 3, 0, PLR_FORMAT_RGBA8};
        const PackedFormattedTextures r = packSceneTexturesFormatted(&same, 1, uvs.data(), 3, m, 3, scene.vertexCounts.data(), 3, scene.drawCount);
        CHECK(!r.compressed && r.texels == q.texels && r.textures == q.textures && r.materials == q.materials && r.uvs == q.uvs && r.formats == std::vector<uint32_t>({0u}));
    }

    int code = 0;
    std::string why;
    auto has = [&](const char* w) { return why.find(w) != std::string::npos; };
    Scene none;
    none.vertexCounts.clear(); none.drawCount = 0;
    why = refusal(none, textures, {}, {}, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("no scene set"));
    why = refusal(scene, textures, {uv0.get(), nullptr}, materials, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mesh count 2") && has("mesh count 3"));
    why = refusal(scene, textures, uvs, {materials[0], materials[1]}, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("draw count 2") && has("draw count 3"));
    {
        std::vector<SceneTextureData> t = textures;
        t[1].format = PLR_FORMAT_RG8;
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("unknown format") && has("texture 1") && has("format 1"));
        t = textures;
        t[4].format = 77;
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("unknown format") && has("texture 4") && has("format 77"));
        t = textures;
        t[1].mipCount = 0;
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("mip_count 0 on a compressed texture") && has("texture 1"));
        t = textures;
        t[1].bytes = n1 - 8;
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("bytes mismatch") && has("texture 1") && has("has 40 bytes") && has("hold 48"));
        t = textures;
        t[3].bytes = n3 + 16;
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("bytes mismatch") && has("texture 3"));
        t = textures;
        t[0].bytes = 18 * 4; // an RGBA8 entry with mip_count 0 gives level 0 alone
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("bytes mismatch") && has("texture 0") && has("hold 60"));
    }
    for (uint32_t bad : {0u, 16385u}) {
        std::vector<SceneTextureData> t = textures;
        t[1].width = bad;
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("texture size out of range") && has("texture 1"));
        t = textures;
        t[4].height = bad;
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("texture size out of range") && has("texture 4"));
    }
    {
        std::vector<SceneTextureData> t = textures;
        t[1].mipCount = 4; // 5 x 7 has 3
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("too many mips") && has("texture 1") && has("at most 3"));
        t = textures;
        t[3].data = nullptr;
        why = refusal(scene, t, uvs, materials, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("null texels") && has("texture 3"));
        std::vector<SceneMaterial> m = materials;
        m[2].specularTexture = 5;
        why = refusal(scene, textures, uvs, m, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("material texture index out of range") && has("draw 2") && has("texture 5 of 5"));
    }
    {
        // 2^28 words are accepted in principle, more are not: sizes are validated before anything is read, so small blocks stand in for the data. An RGBA8
        // 16384 x 16384 fills the store; the padding in front of a compressed texture counts
        std::vector<SceneTextureData> t = {{t2.get(), (uint64_t)16384 * 16384 * 4, 16384, 16384, 1, PLR_FORMAT_RGBA8}, {t4.get(), 16, 1, 1, 1, PLR_FORMAT_BC5}};
        std::vector<SceneMaterial> m = {{0, 1}, {0, 1}, {0, 1}};
        why = refusal(scene, t, uvs, m, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("too many texels") && has("268435460"));
        t = {{t2.get(), (uint64_t)16384 * 16383 * 4, 16384, 16383, 1, PLR_FORMAT_RGBA8}, {t2.get(), (uint64_t)16384 * 4, 16384, 1, 1, PLR_FORMAT_RGBA8}, {t2.get(), 4, 1, 1, 1, PLR_FORMAT_RGBA8}};
        why = refusal(scene, t, uvs, m, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("too many texels") && has("268435457"));
    }
    uv2[5] = std::numeric_limits<float>::quiet_NaN();
    why = refusal(scene, textures, uvs, materials, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("non-finite UV") && has("vertex 2 of mesh 2"));
    uv2[5] = -7.5f;
    why = refusal(scene, textures, uvs, materials, &code);
    CHECK(code == 0);
    std::printf(g_failures ? "scene_bc_check: %d check(s) failed\n" : "scene_bc_check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
