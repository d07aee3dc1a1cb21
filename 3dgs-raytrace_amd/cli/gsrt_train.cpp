// gsrt_train -- train a 3DGS model against rendered or captured views with the library's training session
// (gsrt_trainer, include/gsrt.h), C ABI only.
//
//   gsrt_train --ply IN.ply --views LIST --width W --height H --fovy F --iters N --out OUT.ply
//              [--samples S] [--lambda L] [--densify-every D] [--densify-from A] [--densify-until U]
//              [--opacity-reset-every R] [--grad-threshold T] [--split-scale X] [--min-opacity O] [--capacity C]
//              [--sh-degree-every N] [--max-screen-radius R] [--seed S] [--device D]
//
// LIST holds one "camera_file target.bin" per line: the camera file is gsrt_camera_from_file's (eye and centre, six
// floats), target.bin is H*W*3 float32, the format gsrt_render's --loss-target reads. Views are taken round-robin. Every
// 100 iterations (and at the last) "iter loss l1 ssim n" is printed; at the end the raw model is written with
// gsrt_ply_write. The position rate follows gsrt_lr_expon (1.6e-4 to 1.6e-6 over --iters, delay factor 0.01); the other
// rates are 3DGS's defaults, and so are the densification numbers (every 100 iterations from 500 until 15000 at a
// view-space gradient of 0.0002, a prune below opacity 0.005, an opacity reset to 0.01 every 3000). A densify pass is off
// unless --densify-every is given. --split-scale is 3DGS's percent_dense times the scene extent, which the caller knows.
// --sh-degree-every N: 3DGS's ramp-up, the active SH degree of iteration i (from 1) is i / N, up to 3 or the .ply's (3DGS:
// 1000); 0, the default, keeps degree 3 throughout. --max-screen-radius R: the screen-size prune of a densify pass after
// the first opacity reset, in pixels (3DGS: 20); 0, the default, is off.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/gsrt.h"

namespace {

[[noreturn]] void usage(const char* msg) {
    if (msg) std::fprintf(stderr, "gsrt_train: %s\n", msg);
    std::fprintf(stderr,
                 "usage: gsrt_train --ply IN.ply --views LIST --width W --height H --fovy F --iters N --out OUT.ply\n"
                 "                  [--samples S] [--lambda L] [--densify-every D] [--densify-from A] [--densify-until U]\n"
                 "                  [--opacity-reset-every R] [--grad-threshold T] [--split-scale X] [--min-opacity O]\n"
                 "                  [--capacity C] [--sh-degree-every N] [--max-screen-radius R] [--seed S] [--device D]\n"
                 "  --sh-degree-every N    raise the active SH degree from 0 by one every N iterations (0: degree 3 throughout)\n"
                 "  --max-screen-radius R  after the first opacity reset a densify prunes screen radii above R pixels (0: off)\n");
    std::exit(2);
}

uint32_t to_u32(const char* s, const std::string& flag) {
    char* end = nullptr;
    const unsigned long v = std::strtoul(s, &end, 10);
    if (!*s || !end || *end || v > 0xFFFFFFFFul) usage(("bad value for " + flag).c_str());
    return (uint32_t)v;
}

float to_f32(const char* s, const std::string& flag) {
    char* end = nullptr;
    const float v = std::strtof(s, &end);
    if (!*s || !end || *end) usage(("bad value for " + flag).c_str());
    return v;
}

struct Options {
    std::string ply, views, out;
    uint32_t width = 0, height = 0, iters = 0, samples = 1, device = 0, capacity = 0;
    uint32_t densify_every = 0, densify_from = 500, densify_until = 15000, reset_every = 0, sh_degree_every = 0;
    float fovy = 0.0f, lambda = 0.2f, grad_threshold = 0.0002f, split_scale = 0.01f, min_opacity = 0.005f;
    float max_screen_radius = 0.0f;
    uint64_t seed = 0;
};

struct View {
    gsrt_ubo ubo;
    std::vector<float> target;
};

[[noreturn]] void die(gsrt_ctx* ctx, const char* what, gsrt_status s) {
    std::fprintf(stderr, "gsrt_train: %s: %s (%s)\n", what, gsrt_status_string(s), ctx ? gsrt_last_error(ctx) : "");
    std::exit(1);
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> const char* {
            if (i + 1 >= argc) usage((a + " needs a value").c_str());
            return argv[++i];
        };
        if (a == "--ply") o.ply = val();
        else if (a == "--views") o.views = val();
        else if (a == "--out") o.out = val();
        else if (a == "--width") o.width = to_u32(val(), a);
        else if (a == "--height") o.height = to_u32(val(), a);
        else if (a == "--fovy") o.fovy = to_f32(val(), a);
        else if (a == "--iters") o.iters = to_u32(val(), a);
        else if (a == "--samples") o.samples = to_u32(val(), a);
        else if (a == "--lambda") o.lambda = to_f32(val(), a);
        else if (a == "--densify-every") o.densify_every = to_u32(val(), a);
        else if (a == "--densify-from") o.densify_from = to_u32(val(), a);
        else if (a == "--densify-until") o.densify_until = to_u32(val(), a);
        else if (a == "--opacity-reset-every") o.reset_every = to_u32(val(), a);
        else if (a == "--grad-threshold") o.grad_threshold = to_f32(val(), a);
        else if (a == "--split-scale") o.split_scale = to_f32(val(), a);
        else if (a == "--min-opacity") o.min_opacity = to_f32(val(), a);
        else if (a == "--capacity") o.capacity = to_u32(val(), a);
        else if (a == "--sh-degree-every") o.sh_degree_every = to_u32(val(), a);
        else if (a == "--max-screen-radius") o.max_screen_radius = to_f32(val(), a);
        else if (a == "--seed") o.seed = std::strtoull(val(), nullptr, 10);
        else if (a == "--device") o.device = to_u32(val(), a);
        else if (a == "--help" || a == "-h") usage(nullptr);
        else usage(("unknown option " + a).c_str());
    }
    if (o.ply.empty() || o.views.empty() || o.out.empty()) usage("--ply, --views and --out are needed");
    if (!o.width || !o.height || o.width > 32768 || o.height > 32768) usage("--width and --height must be 1..32768");
    if (!(o.fovy > 0.0f && o.fovy < 180.0f)) usage("--fovy must be in (0, 180)");
    if (!o.iters) usage("--iters must be at least 1");
    if (!o.samples) usage("--samples must be at least 1");
    if (!(o.lambda >= 0.0f && o.lambda <= 1.0f)) usage("--lambda must be in [0, 1]");
    if (!(o.max_screen_radius >= 0.0f)) usage("--max-screen-radius must be >= 0");

    // the model: the reader's activated arrays; the trainer makes them raw
    uint32_t n = 0, degree = 0;
    gsrt_status s = gsrt_ply_info(o.ply.c_str(), &n, &degree);
    if (s != GSRT_OK) die(nullptr, ("cannot parse " + o.ply).c_str(), s);
    if (!n) usage("the .ply holds no Gaussians");
    std::vector<float> center(3ull * n), rot(4ull * n), scale(3ull * n), opacity(n), sh(48ull * n);
    s = gsrt_ply_read(o.ply.c_str(), center.data(), rot.data(), scale.data(), opacity.data(), sh.data());
    if (s != GSRT_OK) die(nullptr, ("cannot read " + o.ply).c_str(), s);
    for (float& x : opacity)  // an opacity of 1 has no logit
        if (x > 0.99f) x = 0.99f;

    // the views
    std::vector<View> views;
    {
        std::ifstream list(o.views);
        if (!list) usage(("cannot open " + o.views).c_str());
        std::string line;
        const size_t floats = 3ull * o.width * o.height;
        while (std::getline(list, line)) {
            std::istringstream is(line);
            std::string cam, tgt;
            if (!(is >> cam)) continue;
            if (!(is >> tgt)) usage(("a line of " + o.views + " is not \"camera_file target.bin\"").c_str());
            View v;
            s = gsrt_camera_from_file(cam.c_str(), o.fovy, o.width, o.height, 1.0f, o.samples, 16, &v.ubo);
            if (s != GSRT_OK) die(nullptr, ("cannot read the camera " + cam).c_str(), s);
            v.target.resize(floats);
            FILE* f = std::fopen(tgt.c_str(), "rb");
            const bool ok = f && std::fread(v.target.data(), sizeof(float), floats, f) == floats;
            if (f) std::fclose(f);
            if (!ok) die(nullptr, ("cannot read H*W*3 floats from " + tgt).c_str(), GSRT_E_IO);
            views.push_back(std::move(v));
        }
        if (views.empty()) usage(("no views in " + o.views).c_str());
    }

    gsrt_ctx* ctx = nullptr;
    if ((s = gsrt_create(&ctx, (int)o.device)) != GSRT_OK) die(nullptr, "gsrt_create", s);
    const uint32_t capacity = o.capacity ? o.capacity : (o.densify_every ? 4 * n : n);
    if (capacity < n) usage("--capacity is below the model's size");
    gsrt_model_arrays model = {center.data(), rot.data(), scale.data(), opacity.data(), sh.data(), nullptr, 0};
    gsrt_trainer* tr = nullptr;
    if ((s = gsrt_trainer_create(ctx, &model, n, capacity, &tr)) != GSRT_OK) die(ctx, "gsrt_trainer_create", s);

    gsrt_frame_loss_params loss{};
    loss.lambda = o.lambda;
    loss.alpha_min = 1.0f / 255.0f;
    gsrt_adam_params adam{};
    adam.lr_rot = 1e-3f, adam.lr_scale = 5e-3f, adam.lr_opacity = 5e-2f, adam.lr_sh_dc = 2.5e-3f, adam.lr_sh_rest = 1.25e-4f;
    adam.beta1 = 0.9f, adam.beta2 = 0.999f, adam.eps = 1e-15f;
    adam.flags = GSRT_ADAM_SPARSE;
    gsrt_densify_params dens{};
    dens.grad_threshold = o.grad_threshold, dens.split_scale = o.split_scale, dens.min_opacity = o.min_opacity;
    dens.shrink = 1.6f;

    const uint32_t top_degree = degree < 3 ? degree : 3;
    bool was_reset = false;
    for (uint32_t it = 0; it < o.iters; ++it) {
        const View& v = views[it % views.size()];
        if (o.sh_degree_every) {
            const uint32_t d = (it + 1) / o.sh_degree_every;
            if ((s = gsrt_trainer_set_sh_degree(tr, d < top_degree ? d : top_degree)) != GSRT_OK) die(ctx, "gsrt_trainer_set_sh_degree", s);
        }
        if ((s = gsrt_lr_expon(1.6e-4f, 1.6e-6f, 0.01f, 0, o.iters, it, &adam.lr_center)) != GSRT_OK) die(ctx, "gsrt_lr_expon", s);
        float sc[GSRT_FRAME_LOSS_SCALARS];
        if ((s = gsrt_trainer_step(tr, &v.ubo, 0, v.target.data(), 3, nullptr, nullptr, &loss, &adam, sc)) != GSRT_OK)
            die(ctx, "gsrt_trainer_step", s);
        const uint32_t done = it + 1;
        if (o.densify_every && done >= o.densify_from && done <= o.densify_until && done % o.densify_every == 0) {
            uint32_t rows = 0;
            s = gsrt_trainer_densify_screen(tr, &dens, was_reset ? o.max_screen_radius : 0.0f, o.seed, &rows);
            if (s == GSRT_E_ARG)  // over the capacity (or nothing left): the model stays as it is
                std::fprintf(stderr, "gsrt_train: iteration %u: no densify (%s)\n", done, gsrt_last_error(ctx));
            else if (s != GSRT_OK)
                die(ctx, "gsrt_trainer_densify", s);
        }
        if (o.reset_every && done % o.reset_every == 0 && done < o.iters) {
            if ((s = gsrt_trainer_opacity_reset(tr, 0.01f)) != GSRT_OK) die(ctx, "gsrt_trainer_opacity_reset", s);
            was_reset = true;
        }
        if (done % 100 == 0 || done == o.iters) {
            gsrt_trainer_info(tr, &n, nullptr, nullptr);
            std::printf("%u %.6f %.6f %.6f %u\n", done, (double)sc[0], (double)sc[1], (double)sc[2], n);
        }
    }

    gsrt_trainer_info(tr, &n, nullptr, nullptr);
    center.resize(3ull * n), rot.resize(4ull * n), scale.resize(3ull * n), opacity.resize(n), sh.resize(48ull * n);
    gsrt_model_arrays raw = {center.data(), rot.data(), scale.data(), opacity.data(), sh.data(), nullptr, 0};
    if ((s = gsrt_trainer_download(tr, &raw, nullptr)) != GSRT_OK) die(ctx, "gsrt_trainer_download", s);
    if ((s = gsrt_ply_write(o.out.c_str(), n, &raw)) != GSRT_OK) die(ctx, ("cannot write " + o.out).c_str(), s);
    gsrt_trainer_destroy(tr);
    gsrt_destroy(ctx);
    return 0;
}
