// gen_frame_refusals.cpp -- writes the reference of tests/test_frame_refusal_host.py: what check_render_args of commit
// e1f9c6a (the last one with a hand-written refusal block per flag) answers over the whole product of modes, callers and
// scene facts. Plain C++, no HIP, no library:
//
//   g++ -std=c++17 -o gen tests/golden/gen_frame_refusals.cpp && ./gen | python tests/test_frame_refusal_host.py
//
// (the test module, run as a script, packs this program's lines into tests/golden/frame_refusals.npz). The text between
// the two "verbatim" marks is that commit's 3dgs-raytrace_amd/csrc/gsrt_api.cpp:765-834 unchanged; the few definitions above
// it stand in for the objects it reads, and fail() keeps (status, message) instead of storing the message in a context.
//
// With -DFRAME_REFUSAL_CHECK, linked with csrc/gsrt_plan.cpp, it writes nothing and compares the library's
// gsrt_debug_frame_refusal with that text over the same product instead (exit status 1 on the first difference): the
// stand-alone program to run the refusal function under sanitizers:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -DFRAME_REFUSAL_CHECK -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       -o check tests/golden/gen_frame_refusals.cpp 3dgs-raytrace_amd/csrc/gsrt_plan.cpp && ./check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gsrt_test.h"

struct gsrt_ctx {};
struct gsrt_scene {
    gsrt_ctx* ctx;
    uint32_t ntri;
    bool bvh_built;
    uint32_t feat_channels;
    const float* d_sh;
};
extern "C" uint32_t gsrt_scene_features(const gsrt_scene* sc) { return sc->feat_channels; }
static std::string g_msg;
static gsrt_status fail(gsrt_ctx*, gsrt_status s, const char* msg) {
    g_msg = msg;
    return s;
}

// ---- verbatim: e1f9c6a 3dgs-raytrace_amd/csrc/gsrt_api.cpp:765-834 ----
// grad_call: the caller is gsrt_render_feature_grad(_async), the only entry point that may carry GSRT_FLAG_FEATURE_GRAD,
// or gsrt_render_sh_grad(_async), the only one that may carry GSRT_FLAG_SH_GRAD, or gsrt_render_opacity_grad(_async), the
// only one that may carry GSRT_FLAG_OPACITY_GRAD
enum class GradCall { none, feature, sh, opacity };
static gsrt_status check_render_args(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, GradCall grad_call = GradCall::none) {
    if (!sc || !ubo) return GSRT_E_ARG;
    if (ubo->width == 0 || ubo->height == 0 || ubo->width > 32768 || ubo->height > 32768)
        return fail(sc->ctx, GSRT_E_ARG, "bad frame size");
    if (mode & GSRT_FLAG_OPACITY_GRAD) {  // a whole COR colour frame that scatters its gradient to the opacities it blends
        const char* why = nullptr;
        if (grad_call != GradCall::opacity)
            why = "GSRT_FLAG_OPACITY_GRAD: only through gsrt_render_opacity_grad (the gradient image goes there)";
        else if ((mode & 0xffu) != GSRT_MODE_COR) why = "GSRT_FLAG_OPACITY_GRAD: COR frames only";
        else if (mode & GSRT_FLAG_STATS) why = "GSRT_FLAG_OPACITY_GRAD: not with GSRT_FLAG_STATS";
        else if (mode & GSRT_FLAG_OUT_DUMP8) why = "GSRT_FLAG_OPACITY_GRAD: not with GSRT_FLAG_OUT_DUMP8";
        else if (mode & GSRT_FLAG_DEPTH) why = "GSRT_FLAG_OPACITY_GRAD: not with GSRT_FLAG_DEPTH";
        else if (mode & GSRT_FLAG_FEATURES) why = "GSRT_FLAG_OPACITY_GRAD: not with GSRT_FLAG_FEATURES";
        else if (mode & GSRT_FLAG_FEATURE_GRAD) why = "GSRT_FLAG_OPACITY_GRAD: not with GSRT_FLAG_FEATURE_GRAD";
        else if (mode & GSRT_FLAG_SH_GRAD) why = "GSRT_FLAG_OPACITY_GRAD: not with GSRT_FLAG_SH_GRAD";
        else if (sc->ntri) why = "GSRT_FLAG_OPACITY_GRAD: not for a scene with a triangle mesh";
        if (why) return fail(sc->ctx, GSRT_E_ARG, why);
    }
    if (mode & GSRT_FLAG_SH_GRAD) {  // a whole COR colour frame that scatters its gradient to the SH rows it blends
        const char* why = nullptr;
        if (grad_call != GradCall::sh) why = "GSRT_FLAG_SH_GRAD: only through gsrt_render_sh_grad (the gradient image goes there)";
        else if ((mode & 0xffu) != GSRT_MODE_COR) why = "GSRT_FLAG_SH_GRAD: COR frames only";
        else if (mode & GSRT_FLAG_STATS) why = "GSRT_FLAG_SH_GRAD: not with GSRT_FLAG_STATS";
        else if (mode & GSRT_FLAG_OUT_DUMP8) why = "GSRT_FLAG_SH_GRAD: not with GSRT_FLAG_OUT_DUMP8";
        else if (mode & GSRT_FLAG_DEPTH) why = "GSRT_FLAG_SH_GRAD: not with GSRT_FLAG_DEPTH";
        else if (mode & GSRT_FLAG_FEATURES) why = "GSRT_FLAG_SH_GRAD: not with GSRT_FLAG_FEATURES";
        else if (mode & GSRT_FLAG_FEATURE_GRAD) why = "GSRT_FLAG_SH_GRAD: not with GSRT_FLAG_FEATURE_GRAD";
        else if (sc->ntri) why = "GSRT_FLAG_SH_GRAD: not for a scene with a triangle mesh";
        if (why) return fail(sc->ctx, GSRT_E_ARG, why);
    }
    if (mode & GSRT_FLAG_FEATURE_GRAD) {  // a whole COR frame that scatters a gradient image to the Gaussians it blends
        const char* why = nullptr;
        if (grad_call != GradCall::feature) why = "GSRT_FLAG_FEATURE_GRAD: only through gsrt_render_feature_grad (the gradient image goes there)";
        else if ((mode & 0xffu) != GSRT_MODE_COR) why = "GSRT_FLAG_FEATURE_GRAD: COR frames only";
        else if (mode & GSRT_FLAG_STATS) why = "GSRT_FLAG_FEATURE_GRAD: not with GSRT_FLAG_STATS";
        else if (mode & GSRT_FLAG_OUT_DUMP8) why = "GSRT_FLAG_FEATURE_GRAD: not with GSRT_FLAG_OUT_DUMP8";
        else if (mode & GSRT_FLAG_DEPTH) why = "GSRT_FLAG_FEATURE_GRAD: not with GSRT_FLAG_DEPTH";
        else if (mode & GSRT_FLAG_FEATURES) why = "GSRT_FLAG_FEATURE_GRAD: not with GSRT_FLAG_FEATURES";
        else if (sc->ntri) why = "GSRT_FLAG_FEATURE_GRAD: not for a scene with a triangle mesh";
        if (why) return fail(sc->ctx, GSRT_E_ARG, why);
    }
    if (mode & GSRT_FLAG_DEPTH) {  // a whole COR frame's second output; the counting pass and dump codes carry none
        if ((mode & 0xffu) != GSRT_MODE_COR) return fail(sc->ctx, GSRT_E_ARG, "GSRT_FLAG_DEPTH: COR frames only");
        if (mode & GSRT_FLAG_STATS) return fail(sc->ctx, GSRT_E_ARG, "GSRT_FLAG_DEPTH: not with GSRT_FLAG_STATS");
        if (mode & GSRT_FLAG_OUT_DUMP8) return fail(sc->ctx, GSRT_E_ARG, "GSRT_FLAG_DEPTH: not with GSRT_FLAG_OUT_DUMP8");
    }
    if (mode & GSRT_FLAG_FEATURES) {  // a whole COR frame that blends the feature table instead of colour
        if ((mode & 0xffu) != GSRT_MODE_COR) return fail(sc->ctx, GSRT_E_ARG, "GSRT_FLAG_FEATURES: COR frames only");
        if (mode & GSRT_FLAG_STATS) return fail(sc->ctx, GSRT_E_ARG, "GSRT_FLAG_FEATURES: not with GSRT_FLAG_STATS");
        if (mode & GSRT_FLAG_OUT_DUMP8) return fail(sc->ctx, GSRT_E_ARG, "GSRT_FLAG_FEATURES: not with GSRT_FLAG_OUT_DUMP8");
        if (mode & GSRT_FLAG_DEPTH) return fail(sc->ctx, GSRT_E_ARG, "GSRT_FLAG_FEATURES: not with GSRT_FLAG_DEPTH");
    }
    if ((mode & 0xffu) > GSRT_MODE_COR ||
        (mode & ~(0xffu | GSRT_FLAG_LUT | GSRT_FLAG_STATS | GSRT_FLAG_DEPTH | GSRT_FLAG_FEATURES | GSRT_FLAG_FEATURE_GRAD |
                  GSRT_FLAG_SH_GRAD | GSRT_FLAG_OPACITY_GRAD)))
        return fail(sc->ctx, GSRT_E_ARG, "bad mode");
    if ((mode & 0xffu) == GSRT_MODE_COR && ubo->samples == 0) return fail(sc->ctx, GSRT_E_ARG, "samples == 0");
    if (!sc->bvh_built) return fail(sc->ctx, GSRT_E_STATE, "render before gsrt_build_bvh");
    if (sc->ntri && (mode & 0xffu) != GSRT_MODE_REF)
        return fail(sc->ctx, GSRT_E_ARG, "triangle meshes are co-traced in REF mode only");
    if ((mode & GSRT_FLAG_FEATURES) && !gsrt_scene_features(sc))
        return fail(sc->ctx, GSRT_E_STATE, "GSRT_FLAG_FEATURES: the scene has no feature table (gsrt_scene_set_features)");
    if ((mode & GSRT_FLAG_SH_GRAD) && !sc->d_sh)
        return fail(sc->ctx, GSRT_E_STATE, "GSRT_FLAG_SH_GRAD: the scene has no SH rows (gsrt_scene_set_sh)");
    return GSRT_OK;
}
// ---- end of the verbatim text ----

int main() {
    // The product, in the order the test enumerates it: pass {samples 1 and built, samples 0, not built} x mode low byte
    // {REF, COR, COR + 1} x the 512 combinations of the bits 0x100 .. 0x10000 x caller {none, feature, sh, opacity} x
    // ntri {0, 1} x feature table {0, 1} x SH rows {0, 1}.
    gsrt_ctx ctx;
    static const float sh_rows[48] = {};
    std::map<std::pair<int, std::string>, uint32_t> ids;
    std::vector<std::pair<int, std::string>> answers;
    std::vector<uint32_t> index;
    for (uint32_t pass = 0; pass < 3; ++pass)
        for (uint32_t low = 0; low < 3; ++low)
            for (uint32_t bits = 0; bits < 512; ++bits)
                for (uint32_t caller = 0; caller < 4; ++caller)
                    for (uint32_t facts = 0; facts < 8; ++facts) {
                        const uint32_t mode = low | bits << 8, ntri = facts >> 2 & 1u, feat = facts >> 1 & 1u, sh = facts & 1u;
                        const uint32_t samples = pass == 1 ? 0u : 1u;
                        const bool built = pass != 2;
                        gsrt_scene sc{&ctx, ntri, built, feat ? 3u : 0u, sh ? sh_rows : nullptr};
                        gsrt_ubo ubo;
                        std::memset(&ubo, 0, sizeof ubo);
                        ubo.width = ubo.height = 16;
                        ubo.samples = samples;
                        g_msg.clear();
                        const gsrt_status s = check_render_args(&sc, &ubo, mode, (GradCall)caller);
#ifdef FRAME_REFUSAL_CHECK
                        char msg[256];
                        const gsrt_status t = gsrt_debug_frame_refusal(mode, caller, samples, built, ntri, (int)feat, (int)sh,
                                                                       msg, sizeof msg);
                        if (t != s || g_msg != msg) {
                            std::fprintf(stderr, "mode 0x%x caller %u samples %u built %d facts %u: %d \"%s\", not %d \"%s\"\n",
                                         mode, caller, samples, (int)built, facts, (int)t, msg, (int)s, g_msg.c_str());
                            return 1;
                        }
#endif
                        const auto key = std::make_pair((int)s, g_msg);
                        auto it = ids.find(key);
                        if (it == ids.end()) {
                            it = ids.emplace(key, (uint32_t)answers.size()).first;
                            answers.push_back(key);
                        }
                        index.push_back(it->second);
                    }
#ifdef FRAME_REFUSAL_CHECK
    std::fprintf(stderr, "%zu cases, %zu distinct answers: all equal\n", index.size(), answers.size());
#else
    // the distinct answers "status<TAB>message" in the order they first appear, an empty line, then one index per case
    for (const auto& a : answers) std::printf("%d\t%s\n", a.first, a.second.c_str());
    std::printf("\n");
    for (uint32_t i : index) std::printf("%u\n", i);
#endif
    return 0;
}
