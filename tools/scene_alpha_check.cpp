// Stand-alone check of the scene alpha cutoff validation and packing (csrc/frontend/scene_packing.cpp) for a sanitizer run on the CPU; no GPU and no backend:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/scene_alpha_check.cpp plainrenderer_amd/csrc/frontend/scene_packing.cpp -o scene_alpha_check
//   ./scene_alpha_check
// It packs cutoffs for scenes of several draw counts, compares every packed word with its source, and sends each kind of invalid input through the validation:
// every refusal must name its cause and none may read outside the caller's array (a heap block of exactly the stated size, so the sanitizer sees an overrun).
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../plainrenderer_amd/csrc/device/depth_prepass_raster.h"
#include "../plainrenderer_amd/csrc/frontend/frame_pipeline.h"

using namespace plrhost;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

// `count` cutoffs in a heap block of exactly that size
static std::unique_ptr<uint32_t[]> block(uint32_t count, uint32_t salt) {
    std::unique_ptr<uint32_t[]> b(new uint32_t[count]);
    for (uint32_t d = 0; d < count; d++) b[d] = (d * 37u + salt) & 255u;
    return b;
}

static std::string refusal(const uint32_t* cutoffs, uint32_t drawCount, uint32_t sceneDrawCount, uint32_t sceneTextureCount, int* code) {
    try {
        packSceneAlphaCutoffs(cutoffs, drawCount, sceneDrawCount, sceneTextureCount);
    } catch (const FramePipelineRefusal& e) {
        *code = e.code;
        return e.what();
    }
    *code = 0;
    return "";
}

int main() {
    static_assert(plr::prepass::kAlphaCutoffReference == 128u && plr::prepass::kAlphaCutoffOpaque == 0u && plr::prepass::kAlphaCutoffDiscardAll == 256u, "cutoff codes");
    static_assert(sizeof(plr::prepass::AlphaPushConstants) == 16 && plr::prepass::kAlphaCutoffBinding == 10, "pass record");
    for (uint32_t count : {1u, 3u, 64u, 1000u}) {
        std::unique_ptr<uint32_t[]> c = block(count, count);
        c[count - 1] = 255u;
        const PackedAlphaCutoffs p = packSceneAlphaCutoffs(c.get(), count, count, 2);
        CHECK(p.cutoffs.size() == count && std::memcmp(p.cutoffs.data(), c.get(), (size_t)count * 4u) == 0 && p.tested);
    }
    {
        std::unique_ptr<uint32_t[]> zeros(new uint32_t[5]());
        const PackedAlphaCutoffs p = packSceneAlphaCutoffs(zeros.get(), 5, 5, 1);
        CHECK(p.cutoffs == std::vector<uint32_t>(5, 0u) && !p.tested); // all opaque: the frame records the pass without the fourth word
        zeros[4] = 1u;
        CHECK(packSceneAlphaCutoffs(zeros.get(), 5, 5, 1).tested);
    }
    int code = 0;
    std::string why;
    auto has = [&](const char* word) { return why.find(word) != std::string::npos; };
    std::unique_ptr<uint32_t[]> c = block(3, 9);
    why = refusal(c.get(), 3, 0, 0, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("no scene set"));
    why = refusal(c.get(), 3, 3, 0, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("no textures set"));
    why = refusal(c.get(), 3, 4, 2, &code); // (the count is refused before a word is read: a 3-word block for a 4-draw scene)
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("cutoff count 3") && has("draw count 4"));
    why = refusal(c.get(), 2, 3, 2, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("cutoff count 2") && has("draw count 3"));
    why = refusal(nullptr, 3, 3, 2, &code);
    CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("cutoffs are null"));
    for (uint32_t bad : {256u, 300u, 0xffffffffu}) {
        c[1] = bad;
        why = refusal(c.get(), 3, 3, 2, &code);
        CHECK(code == PLR_ERR_INVALID_ARGUMENT && has("cutoff out of range") && has("draw 1") && has(std::to_string(bad).c_str()));
    }
    c[1] = 255u;
    why = refusal(c.get(), 3, 3, 2, &code);
    CHECK(code == 0);
    std::printf(g_failures ? "scene_alpha_check: %d check(s) failed\n" : "scene_alpha_check: ok\n", g_failures);
    return g_failures ? 1 : 0;
}
