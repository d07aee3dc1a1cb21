// gsrt_render -- command-line front end of the renderer, taking the reference application's flags
// (RayTracingInVulkan/src/Options.cpp:13-44: --scene --shader-type --width --height --samples --bounces
// --benchmark) so scripts that drove the reference render path (RTV/dump_image.sh, lumibench.sh) can
// drive this one. Written against the C ABI only (include/gsrt.h).
//
//   gsrt_render --scene 33 --shader-type 6 --width 16 --height 16 --samples 1 --bounces 16
//       scene 33 (SceneList.cpp:108-128, the two Gaussians of GaussSplat), REF mode, writes the
//       reference-named "<dd-mm-YYYY-HH-MM-SS->SCENE.ppm" (vulkan_ray_tracing.cc:2216-2247)
//   gsrt_render --scene 100 --gaussians 1000000 --sh --width 1920 --height 1080 --samples 4 --mode cor
//       synthetic front-facing cloud, COR mode
//
// Extra flags: --mode ref|cor, --lut, --gaussians N, --seed S, --sh, --camera FILE (.camera: eye, centre),
// --fov DEG, --out PATH (PPM), --binary PATH (image.binary records), --text PATH (dump_image.sh lines),
// --ply PATH (3DGS scene: COR mode, camera from --camera or looking down -z from the origin), --no-dump,
// --device D, --frames F (with --benchmark: frames timed), --stats, --depth FILE (COR: the frame's expected depth,
// GSRT_FLAG_DEPTH, as a one-channel PFM; a usage error with --mode ref or --stats), --features FILE --feature-channels C
// (raw little-endian float32, n*C values: the scene's feature table) with --features-out FILE (COR: the feature frame,
// GSRT_FLAG_FEATURES, as raw float32 H*W*C, and FILE.pfm when C is 1 or 3; usage errors: --mode ref, --stats, --depth,
// C outside 1..16, one option of the pair without the other), and the gradient runs (COR: one gradient frame, an upstream
// gradient image in as raw float32, a table's gradient out as raw float32, no image dumped; kGradOptions):
// --feature-grad FILE --feature-channels C --feature-grad-out FILE (gsrt_render_feature_grad: W*H*C in, n*C out),
// --sh-grad FILE --sh-grad-out FILE (gsrt_render_sh_grad, a scene with SH rows: the RGBA frame's gradient W*H*4 in, n*48
// laid out [gauss][coef][rgb] out), --opacity-grad FILE --opacity-grad-out FILE (gsrt_render_opacity_grad: W*H*4 in, n
// out), --splat-grad FILE --splat-grad-out FILE (gsrt_render_splat_grad: W*H*4 in, n*8 out; the library refuses --lut).
// --depth-grad FILE beside the --splat-grad pair (the depth image's gradient, W*H): gsrt_render_splat_depth_grad instead,
// the same table out; without --splat-grad it is a usage error. --pose-grad-out FILE beside the --splat-grad pair: the rows
// chained to the camera (gsrt_pose_grad; with --depth-grad its depth form), the 16 floats of dL/d(model_view) written raw and
// the twist (gsrt_pose_twist) printed; without --splat-grad it is a usage error.
// Their usage errors: --mode ref or a REF-default scene, --stats, --depth, --features, a gradient run listed before
// it, one option without the others, C outside 1..16.
// --loss-target FILE [--loss-lambda L] [--loss-channels 3|4] [--loss-grad-out FILE]: after the frame, its photometric
// loss against the target image (gsrt_image_loss: raw float32, W*H*channels, 3 channels and lambda 0.2 by default); prints
// "loss L l1 A ssim S mse M" and writes the loss's gradient with respect to the frame as raw float32 W*H*4, the file
// --splat-grad, --sh-grad and --opacity-grad read. Usage errors: a gradient run (it renders no frame), the other
// --loss options without --loss-target, channels not 3 or 4, lambda outside [0, 1].
// --loss-mask FILE (W*H weights), --loss-background r,g,b, --loss-depth-target FILE (W*H depths; with --depth, whose frame
// supplies the premultiplied depth) [--loss-depth-weight w (1 by default)] [--loss-depth-grad-out FILE], all beside
// --loss-target: the loss is gsrt_frame_loss's instead, the line printed gains "depth_l1 D depth_samples K", and the two
// gradients written are what --splat-grad and --depth-grad read. Usage errors: any of them without --loss-target, a
// background that is not three numbers, --loss-depth-target without --depth, the depth weight or gradient without
// --loss-depth-target, --loss-depth-grad-out without --loss-grad-out.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gsrt_test.h"  // gsrt_synth_cloud: the synthetic clouds of --benchmark

namespace {

struct Options {
    int scene = 33;
    int shader_type = 6;
    uint32_t width = 16, height = 16, samples = 1, bounces = 16;
    bool benchmark = false;
    std::string mode;  // empty: REF for scene 33 / 101, COR for scene 100
    bool lut = false, sh = false, stats = false, no_dump = false;
    uint32_t gaussians = 10000, seed = 42, frames = 10;
    int device = 0;
    float fov = 0.0f;  // 0: scene default
    std::string camera, out, binary, text, ply, depth, features, features_out, feature_grad, feature_grad_out;
    std::string sh_grad, sh_grad_out, opacity_grad, opacity_grad_out, splat_grad, splat_grad_out, depth_grad, pose_grad_out;
    uint32_t feature_channels = 0;
    bool feature_channels_given = false;
    std::string loss_target, loss_grad_out;
    float loss_lambda = 0.2f;
    uint32_t loss_channels = 3;
    bool loss_options_given = false;  // --loss-lambda, --loss-channels or --loss-grad-out
    std::string loss_mask, loss_depth_target, loss_depth_grad_out;  // any of these five: gsrt_frame_loss
    float loss_background[3] = {0.0f, 0.0f, 0.0f}, loss_depth_weight = 1.0f;
    bool loss_background_given = false, loss_depth_weight_given = false;
};

// A gradient run, --NAME FILE with --NAME-out FILE: the upstream gradient image (raw float32, W*H*image_channels) in, the
// table's gradient (raw float32, n*table_floats) out; 0 for either: --feature-channels, which the pair then needs. Oldest
// first: a pair cannot be combined with one before it.
struct GradOption {
    const char* name;
    std::string Options::*in, Options::*out;
    uint32_t image_channels, table_floats;
    gsrt_status (*call)(gsrt_scene*, const gsrt_ubo*, uint32_t mode, const float* gimg, uint32_t channels, float* gtab);
};
const GradOption kGradOptions[] = {
    {"--feature-grad", &Options::feature_grad, &Options::feature_grad_out, 0, 0,
     [](gsrt_scene* s, const gsrt_ubo* u, uint32_t m, const float* g, uint32_t c, float* t) {
         return gsrt_render_feature_grad(s, u, m, 0, g, c, t, 0);
     }},
    {"--sh-grad", &Options::sh_grad, &Options::sh_grad_out, 4, 48,
     [](gsrt_scene* s, const gsrt_ubo* u, uint32_t m, const float* g, uint32_t, float* t) {
         return gsrt_render_sh_grad(s, u, m, 0, g, t, 0);
     }},
    {"--opacity-grad", &Options::opacity_grad, &Options::opacity_grad_out, 4, 1,
     [](gsrt_scene* s, const gsrt_ubo* u, uint32_t m, const float* g, uint32_t, float* t) {
         return gsrt_render_opacity_grad(s, u, m, 0, g, t, 0);
     }},
    {"--splat-grad", &Options::splat_grad, &Options::splat_grad_out, 4, 8,
     [](gsrt_scene* s, const gsrt_ubo* u, uint32_t m, const float* g, uint32_t, float* t) {
         return gsrt_render_splat_grad(s, u, m, 0, g, t, 0);
     }},
};
bool given(const Options& o, const GradOption& g) { return !(o.*g.in).empty() || !(o.*g.out).empty(); }

[[noreturn]] void usage(const char* msg) {
    if (msg) std::fprintf(stderr, "gsrt_render: %s\n", msg);
    std::fprintf(stderr,
                 "usage: gsrt_render [--scene 33|100|101] [--shader-type N] [--width W] [--height H] [--samples S]\n"
                 "                   [--bounces B] [--benchmark] [--mode ref|cor] [--lut] [--gaussians N] [--seed S]\n"
                 "                   [--sh] [--camera FILE] [--fov DEG] [--out PPM] [--binary FILE] [--no-dump]\n"
                 "                   [--text FILE] [--ply FILE] [--device D] [--frames F] [--stats]\n"
                 "                   [--depth PFM] [--features FILE --feature-channels C --features-out FILE]\n"
                 "                   [--feature-grad FILE --feature-channels C --feature-grad-out FILE]\n"
                 "                   [--sh-grad FILE --sh-grad-out FILE]\n"
                 "                   [--opacity-grad FILE --opacity-grad-out FILE]\n"
                 "                   [--splat-grad FILE --splat-grad-out FILE] [--depth-grad FILE]\n"
                 "                   [--pose-grad-out FILE]\n"
                 "                   [--loss-target FILE [--loss-lambda L] [--loss-channels 3|4] [--loss-grad-out FILE]\n"
                 "                    [--loss-mask FILE] [--loss-background r,g,b]\n"
                 "                    [--loss-depth-target FILE [--loss-depth-weight w] [--loss-depth-grad-out FILE]]]\n");
    std::exit(2);
}

uint32_t to_u32(const char* s, const char* flag) {
    char* end = nullptr;
    const unsigned long v = std::strtoul(s, &end, 10);
    if (!end || *end || v > 0xFFFFFFFFul) usage((std::string("bad value for ") + flag).c_str());
    return (uint32_t)v;
}

Options parse(int argc, char** argv) {
    Options o;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> const char* {
            if (i + 1 >= argc) usage((a + " needs a value").c_str());
            return argv[++i];
        };
        if (a == "--scene") o.scene = (int)to_u32(val(), "--scene");
        else if (a == "--shader-type") o.shader_type = (int)to_u32(val(), "--shader-type");
        else if (a == "--width") o.width = to_u32(val(), "--width");
        else if (a == "--height") o.height = to_u32(val(), "--height");
        else if (a == "--samples") o.samples = to_u32(val(), "--samples");
        else if (a == "--bounces") o.bounces = to_u32(val(), "--bounces");
        else if (a == "--benchmark") o.benchmark = true;
        else if (a == "--mode") o.mode = val();
        else if (a == "--lut") o.lut = true;
        else if (a == "--sh") o.sh = true;
        else if (a == "--stats") o.stats = true;
        else if (a == "--no-dump") o.no_dump = true;
        else if (a == "--gaussians") o.gaussians = to_u32(val(), "--gaussians");
        else if (a == "--seed") o.seed = to_u32(val(), "--seed");
        else if (a == "--frames") o.frames = to_u32(val(), "--frames");
        else if (a == "--device") o.device = (int)to_u32(val(), "--device");
        else if (a == "--fov") o.fov = std::strtof(val(), nullptr);
        else if (a == "--camera") o.camera = val();
        else if (a == "--out") o.out = val();
        else if (a == "--binary") o.binary = val();
        else if (a == "--text") o.text = val();
        else if (a == "--ply") o.ply = val();
        else if (a == "--depth") o.depth = val();
        else if (a == "--features") o.features = val();
        else if (a == "--features-out") o.features_out = val();
        else if (a == "--feature-grad") o.feature_grad = val();
        else if (a == "--feature-grad-out") o.feature_grad_out = val();
        else if (a == "--sh-grad") o.sh_grad = val();
        else if (a == "--sh-grad-out") o.sh_grad_out = val();
        else if (a == "--opacity-grad") o.opacity_grad = val();
        else if (a == "--opacity-grad-out") o.opacity_grad_out = val();
        else if (a == "--splat-grad") o.splat_grad = val();
        else if (a == "--splat-grad-out") o.splat_grad_out = val();
        else if (a == "--depth-grad") o.depth_grad = val();
        else if (a == "--pose-grad-out") o.pose_grad_out = val();
        else if (a == "--feature-channels") { o.feature_channels = to_u32(val(), "--feature-channels"); o.feature_channels_given = true; }
        else if (a == "--loss-target") o.loss_target = val();
        else if (a == "--loss-lambda") { o.loss_lambda = std::strtof(val(), nullptr); o.loss_options_given = true; }
        else if (a == "--loss-channels") { o.loss_channels = to_u32(val(), "--loss-channels"); o.loss_options_given = true; }
        else if (a == "--loss-grad-out") { o.loss_grad_out = val(); o.loss_options_given = true; }
        else if (a == "--loss-mask") { o.loss_mask = val(); o.loss_options_given = true; }
        else if (a == "--loss-background") {
            float* b = o.loss_background;
            char tail = 0;
            if (std::sscanf(val(), "%f,%f,%f%c", b, b + 1, b + 2, &tail) != 3) usage("--loss-background takes r,g,b");
            o.loss_background_given = o.loss_options_given = true;
        }
        else if (a == "--loss-depth-target") { o.loss_depth_target = val(); o.loss_options_given = true; }
        else if (a == "--loss-depth-weight") { o.loss_depth_weight = std::strtof(val(), nullptr); o.loss_depth_weight_given = o.loss_options_given = true; }
        else if (a == "--loss-depth-grad-out") { o.loss_depth_grad_out = val(); o.loss_options_given = true; }
        else if (a == "--help" || a == "-h") usage(nullptr);
        else usage(("unknown option " + a).c_str());
    }
    if (o.scene != 33 && o.scene != 100 && o.scene != 101) usage("scene must be 33 (GaussSplat), 100 (COR cloud) or 101 (REF cloud)");
    if (o.mode.empty()) o.mode = (o.scene == 100 || !o.ply.empty()) ? "cor" : "ref";
    if (o.mode != "ref" && o.mode != "cor") usage("--mode must be ref or cor");
    if (!o.width || !o.height) usage("empty frame");
    if (!o.depth.empty() && o.mode != "cor") usage("--depth needs --mode cor (REF frames have no blended depth)");
    if (!o.depth.empty() && o.stats) usage("--depth cannot be combined with --stats");
    if (!o.depth_grad.empty() && o.splat_grad.empty()) usage("--depth-grad goes with --splat-grad and --splat-grad-out");
    if (!o.pose_grad_out.empty() && o.splat_grad.empty()) usage("--pose-grad-out goes with --splat-grad and --splat-grad-out");
    for (const GradOption* g = std::end(kGradOptions); g-- != kGradOptions;) {  // newest first
        if (!given(o, *g)) continue;
        const std::string n = g->name;
        auto clash = [&](bool with, const char* other) {
            if (with) usage((n + " cannot be combined with " + other).c_str());
        };
        const bool channels = !g->image_channels;
        if ((o.*g->in).empty() || (o.*g->out).empty() || (channels && !o.feature_channels_given))
            usage((n + (channels ? ", --feature-channels and " : " and ") + n + "-out go together").c_str());
        if (channels && (o.feature_channels < 1 || o.feature_channels > GSRT_MAX_FEATURES)) usage("--feature-channels must be 1..16");
        if (o.mode != "cor") usage((n + " needs --mode cor (REF frames blend nothing)").c_str());
        clash(o.stats, "--stats");
        clash(!o.depth.empty(), "--depth");
        clash(!o.features.empty() || !o.features_out.empty(), "--features");
        for (const GradOption* older = kGradOptions; older != g; ++older) clash(given(o, *older), older->name);
    }
    if (o.loss_target.empty() && o.loss_options_given) usage("--loss-lambda, --loss-channels, --loss-grad-out and the other --loss options go with --loss-target");
    if (!o.loss_target.empty()) {
        if (o.loss_channels != 3 && o.loss_channels != 4) usage("--loss-channels must be 3 or 4");
        if (!(o.loss_lambda >= 0.0f && o.loss_lambda <= 1.0f)) usage("--loss-lambda must be in [0, 1]");
        if (!o.loss_depth_target.empty() && o.depth.empty()) usage("--loss-depth-target needs --depth (the frame's depth image)");
        if (o.loss_depth_target.empty() && (o.loss_depth_weight_given || !o.loss_depth_grad_out.empty()))
            usage("--loss-depth-weight and --loss-depth-grad-out go with --loss-depth-target");
        if (!o.loss_depth_grad_out.empty() && o.loss_grad_out.empty()) usage("--loss-depth-grad-out needs --loss-grad-out");
        for (const GradOption& g : kGradOptions)
            if (given(o, g)) usage((std::string("--loss-target cannot be combined with ") + g.name + " (a gradient run renders no frame)").c_str());
    }
    // (with --feature-grad, --feature-channels is that pair's)
    if (!given(o, kGradOptions[0]) && (!o.features.empty() || !o.features_out.empty() || o.feature_channels_given)) {
        if (o.features.empty() || o.features_out.empty() || !o.feature_channels_given)
            usage("--features, --feature-channels and --features-out go together");
        if (o.feature_channels < 1 || o.feature_channels > GSRT_MAX_FEATURES) usage("--feature-channels must be 1..16");
        if (o.mode != "cor") usage("--features needs --mode cor (REF frames blend nothing)");
        if (o.stats) usage("--features cannot be combined with --stats");
        if (!o.depth.empty()) usage("--features cannot be combined with --depth");
    }
    return o;
}

int check(gsrt_status s, gsrt_ctx* ctx, const char* what) {
    if (s == GSRT_OK) return 0;
    std::fprintf(stderr, "gsrt_render: %s: %s%s%s\n", what, gsrt_status_string(s), ctx ? ": " : "",
                 ctx ? gsrt_last_error(ctx) : "");
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    const Options o = parse(argc, argv);
    gsrt_ctx* ctx = nullptr;
    if (check(gsrt_create(&ctx, o.device), nullptr, "gsrt_create")) return 1;
    int rc = 0;
    gsrt_scene* scene = nullptr;
    gsrt_ubo ubo;
    float mv[16];
    float fov = o.fov;
    float focus = 1.0f;
    if (!o.ply.empty()) {
        rc = check(gsrt_scene_from_ply(ctx, o.ply.c_str(), 1, &scene), ctx, "scene from ply");
        const float eye[3] = {0, 0, 0}, at[3] = {0, 0, -1}, up[3] = {0, 1, 0};
        if (!rc) rc = check(gsrt_lookat(eye, at, up, mv), ctx, "lookat");
        if (fov == 0.0f) fov = 60.0f;
    } else if (o.scene == 33) {
        // SceneList::GaussSplat: G1 mu (0,0,5) scale 1, G2 mu (0,0,3) scale 2, opacity 0.9, identity rotation;
        // camera translate(0,0,-2), 90 degrees, focus distance 2 (SceneList.cpp:108-128)
        const float center[6] = {0, 0, 5, 0, 0, 3}, rot[8] = {1, 0, 0, 0, 1, 0, 0, 0};
        const float scale[6] = {1, 1, 1, 2, 2, 2}, opacity[2] = {0.9f, 0.9f};
        rc = check(gsrt_scene_from_model(ctx, center, rot, scale, opacity, nullptr, 2, &scene), ctx, "scene");
        // ... and model 0, the triangle sphere CreateSphere((200,200,0), 0.5) (SceneList.cpp:123), co-traced in REF
        if (!rc && o.mode == "ref") {
            const float sc[3] = {200.0f, 200.0f, 0.0f};
            std::vector<float> v(3ull * GSRT_SPHERE_VERTICES);
            std::vector<uint32_t> ix(3ull * GSRT_SPHERE_TRIANGLES);
            rc = check(gsrt_sphere_mesh(sc, 0.5f, v.data(), ix.data()), ctx, "sphere mesh");
            if (!rc) rc = check(gsrt_scene_add_mesh(scene, v.data(), GSRT_SPHERE_VERTICES, ix.data(), GSRT_SPHERE_TRIANGLES),
                                ctx, "add mesh");
        }
        std::memset(mv, 0, sizeof mv);
        mv[0] = mv[5] = mv[10] = mv[15] = 1.0f;
        mv[14] = -2.0f;
        if (fov == 0.0f) fov = 90.0f;
        focus = 2.0f;
    } else {
        const uint32_t n = o.gaussians;
        std::vector<float> c(3ull * n), r(4ull * n), s(3ull * n), op(n), sh(o.sh ? 48ull * n : 0);
        const uint32_t kind = o.scene == 100 ? GSRT_SYNTH_COR : GSRT_SYNTH_REF;
        rc = check(gsrt_synth_cloud(kind, n, o.seed, o.sh ? 1 : 0, c.data(), r.data(), s.data(), op.data(),
                                    o.sh ? sh.data() : nullptr), ctx, "synth_cloud");
        if (!rc)
            rc = check(gsrt_scene_from_model(ctx, c.data(), r.data(), s.data(), op.data(), o.sh ? sh.data() : nullptr,
                                             n, &scene), ctx, "scene");
        const float eye[3] = {0, 0, 0}, at[3] = {0, 0, -1}, up[3] = {0, 1, 0};
        if (!rc) rc = check(gsrt_lookat(eye, at, up, mv), ctx, "lookat");
        if (fov == 0.0f) fov = 60.0f;
    }
    if (!rc) {
        if (!o.camera.empty())
            rc = check(gsrt_camera_from_file(o.camera.c_str(), fov, o.width, o.height, focus, o.samples, o.bounces, &ubo),
                       ctx, "camera file");
        else
            rc = check(gsrt_camera_from_modelview(mv, fov, o.width, o.height, focus, o.samples, o.bounces, &ubo), ctx,
                       "camera");
    }
    if (!rc) rc = check(gsrt_build_bvh(scene), ctx, "build_bvh");
    uint32_t mode = o.mode == "ref" ? GSRT_MODE_REF : GSRT_MODE_COR;
    if (o.lut) mode |= GSRT_FLAG_LUT;
    if (o.stats) mode |= GSRT_FLAG_STATS;
    std::vector<float> rgba((size_t)o.width * o.height * 4);
    std::vector<float> depth(o.depth.empty() ? 0 : (size_t)o.width * o.height);
    const GradOption* grad = nullptr;  // the gradient run asked for (parse: at most one)
    for (const GradOption& g : kGradOptions)
        if (given(o, g)) grad = &g;
    if (!rc && !o.depth.empty()) {
        mode |= GSRT_FLAG_DEPTH;
        rc = check(gsrt_render_depth(scene, &ubo, mode, 0, rgba.data(), depth.data()), ctx, "render");
        if (!rc) rc = check(gsrt_dump_pfm(o.depth.c_str(), depth.data(), o.width, o.height, 1), ctx, "dump_pfm");
        if (!rc) std::printf("wrote %s\n", o.depth.c_str());
    } else if (!rc && !o.features.empty()) {
        // the table: n * C raw float32; the frame: H * W * C raw float32 (and a PFM of it when C is 1 or 3)
        const uint32_t C = o.feature_channels;
        std::vector<float> table((size_t)gsrt_scene_size(scene) * C), feat((size_t)o.width * o.height * C);
        FILE* f = std::fopen(o.features.c_str(), "rb");
        const bool whole = f && std::fread(table.data(), sizeof(float), table.size(), f) == table.size() &&
                           std::fgetc(f) == EOF;
        if (f) std::fclose(f);
        if (!whole) {
            std::fprintf(stderr, "gsrt_render: %s: not %zu float32 values (Gaussians x channels)\n", o.features.c_str(),
                         table.size());
            rc = 1;
        }
        if (!rc) rc = check(gsrt_scene_set_features(scene, table.data(), C), ctx, "set_features");
        if (!rc) rc = check(gsrt_render_features(scene, &ubo, mode, 0, rgba.data(), feat.data()), ctx, "render");
        if (!rc) {
            f = std::fopen(o.features_out.c_str(), "wb");
            const bool ok = f && std::fwrite(feat.data(), sizeof(float), feat.size(), f) == feat.size();
            if ((f && std::fclose(f) != 0) || !ok) rc = check(GSRT_E_IO, nullptr, o.features_out.c_str());
        }
        if (!rc) std::printf("wrote %s\n", o.features_out.c_str());
        if (!rc && (C == 1 || C == 3)) {
            const std::string pfm = o.features_out + ".pfm";
            rc = check(gsrt_dump_pfm(pfm.c_str(), feat.data(), o.width, o.height, C), ctx, "dump_pfm");
            if (!rc) std::printf("wrote %s\n", pfm.c_str());
        }
    } else if (!rc && grad) {
        const uint32_t C = grad->image_channels ? grad->image_channels : o.feature_channels;
        const uint32_t T = grad->table_floats ? grad->table_floats : o.feature_channels;
        const std::string &in = o.*grad->in, &out = o.*grad->out;
        std::vector<float> gimg((size_t)o.width * o.height * C), gtab((size_t)gsrt_scene_size(scene) * T);
        FILE* f = std::fopen(in.c_str(), "rb");
        const bool whole = f && std::fread(gimg.data(), sizeof(float), gimg.size(), f) == gimg.size() &&
                           std::fgetc(f) == EOF;
        if (f) std::fclose(f);
        if (!whole) {
            std::fprintf(stderr, "gsrt_render: %s: not %zu float32 values (pixels x %s)\n", in.c_str(), gimg.size(),
                         grad->image_channels ? "4" : "channels");
            rc = 1;
        }
        std::vector<float> gdepth(o.depth_grad.empty() ? 0 : (size_t)o.width * o.height);  // with --splat-grad (parse)
        if (!rc && !gdepth.empty()) {
            f = std::fopen(o.depth_grad.c_str(), "rb");
            const bool all = f && std::fread(gdepth.data(), sizeof(float), gdepth.size(), f) == gdepth.size() &&
                             std::fgetc(f) == EOF;
            if (f) std::fclose(f);
            if (!all) {
                std::fprintf(stderr, "gsrt_render: %s: not %zu float32 values (pixels)\n", o.depth_grad.c_str(), gdepth.size());
                rc = 1;
            }
        }
        if (!rc && !gdepth.empty())
            rc = check(gsrt_render_splat_depth_grad(scene, &ubo, mode, 0, gimg.data(), gdepth.data(), gtab.data(), 0), ctx,
                       "render");
        else if (!rc) rc = check(grad->call(scene, &ubo, mode, gimg.data(), C, gtab.data()), ctx, "render");
        if (!rc) {
            f = std::fopen(out.c_str(), "wb");
            const bool ok = f && std::fwrite(gtab.data(), sizeof(float), gtab.size(), f) == gtab.size();
            if ((f && std::fclose(f) != 0) || !ok) rc = check(GSRT_E_IO, nullptr, out.c_str());
        }
        if (!rc) std::printf("wrote %s\n", out.c_str());
        if (!rc && !o.pose_grad_out.empty()) {  // with --splat-grad (parse): gtab holds the splat rows
            float gmv[16], twist[6];
            rc = check(gsrt_pose_grad(scene, &ubo, gtab.data(), gdepth.empty() ? 0 : 1, gmv), ctx, "pose_grad");
            if (!rc) rc = check(gsrt_pose_twist(ubo.model_view, gmv, twist), ctx, "pose_twist");
            if (!rc) {
                f = std::fopen(o.pose_grad_out.c_str(), "wb");
                const bool ok = f && std::fwrite(gmv, sizeof(float), 16, f) == 16;
                if ((f && std::fclose(f) != 0) || !ok) rc = check(GSRT_E_IO, nullptr, o.pose_grad_out.c_str());
            }
            if (!rc)
                std::printf("wrote %s\ntwist dL/dv %.9g %.9g %.9g dL/dw %.9g %.9g %.9g\n", o.pose_grad_out.c_str(), twist[0],
                            twist[1], twist[2], twist[3], twist[4], twist[5]);
        }
    } else if (!rc) {
        rc = check(gsrt_render(scene, &ubo, mode, 0, rgba.data(), nullptr), ctx, "render");
    }
    if (!rc && o.stats) {
        uint64_t st[8];
        rc = check(gsrt_last_stats(ctx, st, nullptr), ctx, "stats");
        if (!rc)
            std::printf("rays %llu candidates %llu blended %llu terminated %llu rounds %llu tiles %llu\n",
                        (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2],
                        (unsigned long long)st[3], (unsigned long long)st[4], (unsigned long long)st[6]);
    }
    if (!rc && !o.loss_target.empty()) {
        // the target: W * H * channels raw float32; the gradient: W * H * 4 raw float32, what --splat-grad reads
        const size_t px = (size_t)o.width * o.height;
        std::vector<float> target(px * o.loss_channels), gimg(o.loss_grad_out.empty() ? 0 : px * 4);
        FILE* f = std::fopen(o.loss_target.c_str(), "rb");
        const bool whole = f && std::fread(target.data(), sizeof(float), target.size(), f) == target.size() &&
                           std::fgetc(f) == EOF;
        if (f) std::fclose(f);
        if (!whole) {
            std::fprintf(stderr, "gsrt_render: %s: not %zu float32 values (pixels x %u)\n", o.loss_target.c_str(),
                         target.size(), o.loss_channels);
            rc = 1;
        }
        // W * H raw float32 each: the mask and the target depth in, the depth's gradient (what --depth-grad reads) out
        const bool frame_loss = !o.loss_mask.empty() || o.loss_background_given || !o.loss_depth_target.empty();
        std::vector<float> mask(o.loss_mask.empty() ? 0 : px), tdepth(o.loss_depth_target.empty() ? 0 : px);
        std::vector<float> gdepth(o.loss_depth_grad_out.empty() ? 0 : px);
        for (const auto& in : {std::make_pair(&o.loss_mask, &mask), std::make_pair(&o.loss_depth_target, &tdepth)}) {
            if (rc || in.second->empty()) continue;
            f = std::fopen(in.first->c_str(), "rb");
            const bool all = f && std::fread(in.second->data(), sizeof(float), px, f) == px && std::fgetc(f) == EOF;
            if (f) std::fclose(f);
            if (!all) {
                std::fprintf(stderr, "gsrt_render: %s: not %zu float32 values (pixels)\n", in.first->c_str(), px);
                rc = 1;
            }
        }
        float sc[GSRT_FRAME_LOSS_SCALARS] = {0, 0, 0, 0, 0, 0};
        if (!rc && frame_loss) {
            gsrt_frame_loss_params P{};
            P.lambda = o.loss_lambda;
            for (int c = 0; c < 3; ++c) P.background[c] = o.loss_background[c];
            P.depth_weight = tdepth.empty() ? 0.0f : o.loss_depth_weight;
            P.alpha_min = 1.0f / 255.0f;
            P.flags = o.loss_background_given ? GSRT_LOSS_BACKGROUND : 0u;
            rc = check(gsrt_frame_loss(ctx, o.width, o.height, rgba.data(), target.data(), o.loss_channels,
                                       mask.empty() ? nullptr : mask.data(), tdepth.empty() ? nullptr : depth.data(),
                                       tdepth.empty() ? nullptr : tdepth.data(), &P, sc, gimg.empty() ? nullptr : gimg.data(),
                                       gdepth.empty() ? nullptr : gdepth.data()), ctx, "frame_loss");
            if (!rc)
                std::printf("loss %.9g l1 %.9g ssim %.9g mse %.9g depth_l1 %.9g depth_samples %.9g\n", sc[0], sc[1], sc[2],
                            sc[3], sc[4], sc[5]);
        } else if (!rc) {
            rc = check(gsrt_image_loss(ctx, o.width, o.height, rgba.data(), target.data(), o.loss_channels, o.loss_lambda, sc,
                                       gimg.empty() ? nullptr : gimg.data()), ctx, "image_loss");
            if (!rc) std::printf("loss %.9g l1 %.9g ssim %.9g mse %.9g\n", sc[0], sc[1], sc[2], sc[3]);
        }
        if (!rc && !gdepth.empty()) {
            f = std::fopen(o.loss_depth_grad_out.c_str(), "wb");
            const bool ok = f && std::fwrite(gdepth.data(), sizeof(float), gdepth.size(), f) == gdepth.size();
            if ((f && std::fclose(f) != 0) || !ok) rc = check(GSRT_E_IO, nullptr, o.loss_depth_grad_out.c_str());
            if (!rc) std::printf("wrote %s\n", o.loss_depth_grad_out.c_str());
        }
        if (!rc && !gimg.empty()) {
            f = std::fopen(o.loss_grad_out.c_str(), "wb");
            const bool ok = f && std::fwrite(gimg.data(), sizeof(float), gimg.size(), f) == gimg.size();
            if ((f && std::fclose(f) != 0) || !ok) rc = check(GSRT_E_IO, nullptr, o.loss_grad_out.c_str());
            if (!rc) std::printf("wrote %s\n", o.loss_grad_out.c_str());
        }
    }
    if (!rc && o.benchmark) {
        const uint32_t frames = o.frames ? o.frames : 1;
        const uint32_t m = mode & ~(uint32_t)GSRT_FLAG_STATS;
        rc = check(gsrt_synchronize(ctx), ctx, "sync");
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t f = 0; f < frames && !rc; ++f) rc = check(gsrt_render_async(scene, &ubo, m, 0, nullptr, nullptr), ctx, "render");
        if (!rc) rc = check(gsrt_synchronize(ctx), ctx, "sync");
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const double rays = (double)o.width * o.height * o.samples * frames;
        if (!rc) std::printf("%u frames %.3f ms/frame %.1f Mrays/s\n", frames, dt / frames * 1e3, rays / dt / 1e6);
    }
    if (!rc && !o.no_dump && !grad) {  // a gradient run writes its table only
        std::string path = o.out;
        if (path.empty()) {
            char name[128];
            rc = check(gsrt_reference_ppm_name(name, sizeof name), ctx, "ppm name");
            path = name;
        }
        if (!rc) rc = check(gsrt_dump_ppm(path.c_str(), rgba.data(), o.width, o.height), ctx, "dump_ppm");
        if (!rc) std::printf("wrote %s\n", path.c_str());
        if (!rc && !o.binary.empty())
            rc = check(gsrt_dump_image_binary(o.binary.c_str(), rgba.data(), o.width, o.height), ctx, "dump_image_binary");
        if (!rc && !o.text.empty())
            rc = check(gsrt_dump_rgba_text(o.text.c_str(), rgba.data(), o.width, o.height), ctx, "dump_rgba_text");
    }
    if (scene) gsrt_destroy_scene(scene);
    gsrt_destroy(ctx);
    return rc;
}
