// gsrt_trainer.cpp -- the training session (gsrt_trainer_*, include/gsrt.h) and gsrt_lr_expon.
//
// Host code over the library's own entry points: a trainer owns the device arrays of a run and calls the _async forms in
// the order the header gives, with the one gsrt_synchronize a step needs between gsrt_model_step_async and
// gsrt_scene_update. It launches no kernel of its own. Everything per Gaussian is allocated once, for `capacity` rows:
//   two sets of raw, m, v (cur and the other one, which gsrt_trainer_densify writes and then makes cur),
//   two activated sets without SH (act[0]: gsrt_model_activate's output, the densify pass's input; act[1]: its output;
//   an activated model's SH rows are its raw model's, so act[i].sh points into a raw set),
//   the gradient tables (centre 3, cov 6, splat rows 8, SH 48), stats 2, radii 1, noise 6, origin 1, the scene arrays of a step
//   (params 12, aabbs 6), and a few scalars. The frame buffers (rgba, depth, both gradients, staged targets) follow the
//   frame size.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/gsrt_test.h"
#include "gsrt_api_util.hpp"

using gsrt::fail;
using gsrt::is_device_ptr;
using gsrt::model_fields;
using gsrt::ModelField;

struct gsrt_trainer {
    gsrt_ctx* ctx = nullptr;
    gsrt_scene* scene = nullptr;
    uint32_t n = 0, cap = 0, step = 0;
    uint32_t sh_degree = 3;           // the active SH degree of a step
    bool has_sh = false;
    int cur = 0;                      // the buffer set in use
    gsrt_model_arrays raw[2]{}, m[2]{}, v[2]{};
    gsrt_model_arrays act[2]{};       // act[i].sh is set per use
    float *g_center = nullptr, *g_cov = nullptr, *g_splat = nullptr, *g_sh = nullptr;
    float *stats = nullptr, *radii = nullptr, *noise = nullptr, *scalars = nullptr;
    int32_t* origin = nullptr;
    uint32_t* d_n_out = nullptr;
    gsrt_gauss_param* params = nullptr;
    gsrt_aabb* aabbs = nullptr;
    // frame-sized
    size_t px = 0;
    float *rgba = nullptr, *depth = nullptr, *gimg = nullptr, *gdepth = nullptr;
    float *t_target = nullptr, *t_mask = nullptr, *t_depth = nullptr;  // host targets staged
    std::vector<void*> blocks;        // every per-Gaussian allocation, for destroy
};

namespace {

template <class T>
bool dev_alloc(gsrt_trainer* t, T** p, size_t count) {
    if (hipMalloc(p, sizeof(T) * (count ? count : 1)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return false;
    }
    t->blocks.push_back(*p);
    return true;
}

// the arrays that `like` has, for the trainer's capacity
bool alloc_set(gsrt_trainer* t, gsrt_model_arrays& a, const gsrt_model_arrays& like) {
    ModelField f[6];
    const uint32_t nf = model_fields(like, f);
    for (uint32_t i = 0; i < nf; ++i)
        if (!dev_alloc(t, &(a.*f[i].member), (size_t)f[i].floats * t->cap)) return false;
    return true;
}

void free_frame(gsrt_trainer* t) {
    for (float** p : {&t->rgba, &t->depth, &t->gimg, &t->gdepth, &t->t_target, &t->t_mask, &t->t_depth}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    t->px = 0;
}

// the frame buffers for px pixels; regrown only when the frame size changes (after draining what may still use them)
gsrt_status frame_buffers(gsrt_trainer* t, size_t px) {
    if (t->px == px) return GSRT_OK;
    if (gsrt_status s = gsrt_synchronize(t->ctx); s != GSRT_OK) return s;
    free_frame(t);
    const size_t floats[7] = {4 * px, px, 4 * px, px, 4 * px, px, px};
    float** slot[7] = {&t->rgba, &t->depth, &t->gimg, &t->gdepth, &t->t_target, &t->t_mask, &t->t_depth};
    for (int i = 0; i < 7; ++i)
        if (hipMalloc(slot[i], sizeof(float) * floats[i]) != hipSuccess) {
            (void)hipGetLastError();
            *slot[i] = nullptr;
            free_frame(t);
            return fail(t->ctx, GSRT_E_OOM, "gsrt_trainer_step: device allocation of the frame buffers failed");
        }
    t->px = px;
    return GSRT_OK;
}

gsrt_model_arrays with_sh_of(const gsrt_model_arrays& act, const gsrt_model_arrays& raw) {
    gsrt_model_arrays a = act;
    a.sh = raw.sh;  // an activated model's SH rows are its raw model's
    return a;
}

// whether a whole frame of `mode` through `caller` would be refused for the trainer's scene (gsrt_plan.cpp's rule)
gsrt_status frame_ok(gsrt_trainer* t, uint32_t mode, uint32_t caller, uint32_t samples) {
    char msg[256];
    const gsrt_status s =
        gsrt_debug_frame_refusal_any(mode, caller, samples, 1, gsrt_scene_mesh_triangles(t->scene),
                                     gsrt_scene_features(t->scene) != 0, t->has_sh, msg, sizeof msg);
    return s == GSRT_OK ? GSRT_OK : fail(t->ctx, s, std::string("gsrt_trainer_step: ") + msg);
}

// the scene's arrays from the raw model in use: gsrt_model_activate into the step's scene arrays, then the update
gsrt_status scene_follows_raw(gsrt_trainer* t) {
    gsrt_ctx* ctx = t->ctx;
    const gsrt_model_arrays a = with_sh_of(t->act[0], t->raw[t->cur]);
    gsrt_status s = gsrt_model_activate_async(ctx, t->n, &t->raw[t->cur], &a, t->params, t->aabbs);
    if (s == GSRT_OK) s = gsrt_synchronize(ctx);  // gsrt_scene_update reads its source on other streams
    if (s == GSRT_OK) s = gsrt_scene_update(t->scene, t->params, t->aabbs);
    if (s == GSRT_OK) s = gsrt_refit_bvh(t->scene, nullptr);
    return s;
}

}  // namespace

extern "C" {

gsrt_status gsrt_lr_expon(float lr_init, float lr_final, float delay_mult, uint32_t delay_steps, uint32_t max_steps,
                          uint32_t step, float* lr) {
    if (!lr || max_steps == 0) return GSRT_E_ARG;
    if (!(lr_init >= 0.0f) || !(lr_final >= 0.0f) || std::isnan(delay_mult)) return GSRT_E_ARG;
    if ((lr_init == 0.0f) != (lr_final == 0.0f)) return GSRT_E_ARG;
    if (lr_init == 0.0f) {
        *lr = 0.0f;
        return GSRT_OK;
    }
    const auto clamp01 = [](double x) { return x < 0.0 ? 0.0 : x > 1.0 ? 1.0 : x; };
    double delay = 1.0;
    if (delay_steps > 0)
        delay = (double)delay_mult +
                (1.0 - (double)delay_mult) * std::sin(0.5 * M_PI * clamp01((double)step / (double)delay_steps));
    const double t = clamp01((double)step / (double)max_steps);
    *lr = (float)(delay * std::exp(std::log((double)lr_init) * (1.0 - t) + std::log((double)lr_final) * t));
    return GSRT_OK;
}

void gsrt_trainer_destroy(gsrt_trainer* t) {
    if (!t) return;
    (void)hipSetDevice(t->ctx->device);
    (void)gsrt_synchronize(t->ctx);
    if (t->scene) gsrt_destroy_scene(t->scene);
    free_frame(t);
    for (void* p : t->blocks) (void)hipFree(p);
    delete t;
}

gsrt_status gsrt_trainer_create(gsrt_ctx* ctx, const gsrt_model_arrays* model, uint32_t n, uint32_t capacity,
                                gsrt_trainer** out) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = "gsrt_trainer_create: ";
    if (!model || !out) return fail(ctx, GSRT_E_ARG, name + "a NULL pointer");
    if (model->features || model->feature_channels) return fail(ctx, GSRT_E_ARG, name + "a model with features");
    if (n == 0 || capacity < n || capacity > GSRT_MAX_GAUSSIANS)
        return fail(ctx, GSRT_E_ARG, name + "needs 1 <= n <= capacity <= GSRT_MAX_GAUSSIANS");
    if (!model->center || !model->rot_rxyz || !model->scale || !model->opacity) return fail(ctx, GSRT_E_ARG, name + "a NULL array");
    ModelField mf[6];
    const uint32_t nf = model_fields(*model, mf);  // sh only when the model has it
    const bool dev = is_device_ptr(model->center);
    for (uint32_t f = 1; f < nf; ++f)
        if (is_device_ptr(model->*mf[f].member) != dev)
            return fail(ctx, GSRT_E_ARG, name + "the arrays must all be host pointers or all be device pointers");
    (void)hipSetDevice(ctx->device);
    gsrt_trainer* t = new (std::nothrow) gsrt_trainer;
    if (!t) return fail(ctx, GSRT_E_OOM, name + "host allocation failed");
    t->ctx = ctx;
    t->n = n;
    t->cap = capacity;
    t->has_sh = model->sh != nullptr;
    const size_t cap = capacity;
    bool ok = true;
    gsrt_model_arrays no_sh = *model;  // an activated set's SH rows are a raw set's
    no_sh.sh = nullptr;
    for (int i = 0; i < 2 && ok; ++i)
        ok = alloc_set(t, t->raw[i], *model) && alloc_set(t, t->m[i], *model) && alloc_set(t, t->v[i], *model) &&
             alloc_set(t, t->act[i], no_sh);
    ok = ok && dev_alloc(t, &t->g_center, 3 * cap) && dev_alloc(t, &t->g_cov, 6 * cap) && dev_alloc(t, &t->g_splat, 8 * cap) &&
         (!t->has_sh || dev_alloc(t, &t->g_sh, 48 * cap)) && dev_alloc(t, &t->stats, 2 * cap) && dev_alloc(t, &t->radii, cap) &&
         dev_alloc(t, &t->noise, 6 * cap) && dev_alloc(t, &t->scalars, 8) && dev_alloc(t, &t->origin, cap) &&
         dev_alloc(t, &t->d_n_out, 4) && dev_alloc(t, &t->params, cap) && dev_alloc(t, &t->aabbs, cap);
    if (!ok) {
        gsrt_trainer_destroy(t);
        return fail(ctx, GSRT_E_OOM, name + "device allocation failed");
    }
    hipStream_t st = (hipStream_t)gsrt_stream(ctx);
    gsrt_status s = GSRT_OK;
    const auto hip = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && s == GSRT_OK) s = fail(ctx, GSRT_E_DEVICE, name + what + ": " + hipGetErrorString(e));
    };
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    gsrt_model_arrays a0 = with_sh_of(t->act[0], t->raw[0]);
    for (uint32_t f = 0; f < nf; ++f)
        hip(hipMemcpyAsync(a0.*mf[f].member, model->*mf[f].member, sizeof(float) * mf[f].floats * n, kind, st), "upload");
    for (int i = 0; i < 2; ++i)
        for (gsrt_model_arrays* set : {&t->m[i], &t->v[i]})
            for (uint32_t f = 0; f < nf; ++f)
                hip(hipMemsetAsync(set->*mf[f].member, 0, sizeof(float) * mf[f].floats * cap, st), "memset");
    hip(hipMemsetAsync(t->stats, 0, sizeof(float) * 2 * cap, st), "memset");
    hip(hipMemsetAsync(t->radii, 0, sizeof(float) * cap, st), "memset");
    if (s == GSRT_OK) s = gsrt_model_deactivate_async(ctx, n, &a0, &t->raw[0]);
    if (s == GSRT_OK) s = gsrt_synchronize(ctx);  // gsrt_scene_from_model reads a device source at the call
    if (s == GSRT_OK) s = gsrt_scene_from_model(ctx, a0.center, a0.rot_rxyz, a0.scale, a0.opacity, a0.sh, n, &t->scene);
    if (s == GSRT_OK) s = gsrt_build_bvh(t->scene);
    if (s != GSRT_OK) {
        const std::string why = gsrt_last_error(ctx);
        gsrt_trainer_destroy(t);
        return fail(ctx, s, why);
    }
    *out = t;
    return GSRT_OK;
}

gsrt_status gsrt_trainer_step(gsrt_trainer* t, const gsrt_ubo* ubo, uint32_t k, const float* target,
                              uint32_t target_channels, const float* mask, const float* target_depth,
                              const gsrt_frame_loss_params* P, const gsrt_adam_params* adam,
                              float scalars[GSRT_FRAME_LOSS_SCALARS]) {
    if (!t) return GSRT_E_ARG;
    gsrt_ctx* ctx = t->ctx;
    const std::string name = "gsrt_trainer_step: ";
    // ---- everything a call below would refuse, before anything is enqueued
    if (!ubo || !target || !P || !adam) return fail(ctx, GSRT_E_ARG, name + "ubo, target, params or adam is NULL");
    const uint32_t W = ubo->width, H = ubo->height;
    if (W == 0 || H == 0 || W > 32768 || H > 32768) return fail(ctx, GSRT_E_ARG, name + "bad frame size");
    if (target_channels != 3 && target_channels != 4) return fail(ctx, GSRT_E_ARG, name + "target_channels must be 3 or 4");
    gsrt_status s = gsrt::check_frame_loss_params(ctx, name, *P);
    if (s != GSRT_OK) return s;
    gsrt_adam_params A = *adam;
    A.step = t->step + 1;  // the trainer counts
    float ks[GSRT_ADAM_SCALARS];
    if (A.step == 0 || gsrt_adam_scalars(&A, ks) != GSRT_OK) return fail(ctx, GSRT_E_ARG, name + "bad Adam parameters");
    const bool dev = is_device_ptr(target);
    for (const float* p : {mask, target_depth})
        if (p && is_device_ptr(p) != dev)
            return fail(ctx, GSRT_E_ARG, name + "target, mask and target_depth must all be host pointers or all be device pointers");
    if (dev && target_channels == 4 && reinterpret_cast<uintptr_t>(target) % 16u)
        return fail(ctx, GSRT_E_ARG, name + "a 4-channel device target must be 16-byte aligned");
    const bool with_depth = target_depth != nullptr;
    const uint32_t fwd = GSRT_MODE_COR | (with_depth ? GSRT_FLAG_DEPTH : 0u);
    const uint32_t bwd = GSRT_MODE_COR | (with_depth ? GSRT_FLAG_SPLAT_DEPTH_GRAD : GSRT_FLAG_SPLAT_GRAD);
    s = frame_ok(t, fwd, 0, ubo->samples);
    if (s == GSRT_OK) s = frame_ok(t, bwd, with_depth ? 5u : 4u, ubo->samples);
    if (s == GSRT_OK && t->has_sh) s = frame_ok(t, GSRT_MODE_COR | GSRT_FLAG_SH_GRAD, 2, ubo->samples);
    if (s != GSRT_OK) return s;

    // ---- the iteration
    (void)hipSetDevice(ctx->device);
    const size_t px = (size_t)W * H;
    if ((s = frame_buffers(t, px)) != GSRT_OK) return s;
    hipStream_t st = (hipStream_t)gsrt_stream(ctx);
    const float *d_target = target, *d_mask = mask, *d_tdepth = target_depth;
    if (!dev) {
        const auto stage = [&](float* d, const float* h, size_t floats) -> const float* {
            if (!h) return nullptr;
            if (s == GSRT_OK && hipMemcpyAsync(d, h, sizeof(float) * floats, hipMemcpyHostToDevice, st) != hipSuccess)
                s = fail(ctx, GSRT_E_DEVICE, name + "upload of a target failed");
            return d;
        };
        d_target = stage(t->t_target, target, target_channels * px);
        d_mask = stage(t->t_mask, mask, px);
        d_tdepth = stage(t->t_depth, target_depth, px);
        if (s != GSRT_OK) return s;
    }
    gsrt_scene* sc = t->scene;
    const gsrt_model_arrays &raw = t->raw[t->cur], &m = t->m[t->cur], &v = t->v[t->cur];
    const gsrt_model_grads grads = {t->g_center, t->g_cov, t->g_splat, t->has_sh ? t->g_sh : nullptr, nullptr};
    if (with_depth) {
        s = gsrt_render_depth_async(sc, ubo, GSRT_MODE_COR, k, t->rgba, t->depth);
        if (s == GSRT_OK)
            s = gsrt_frame_loss_async(ctx, W, H, t->rgba, d_target, target_channels, d_mask, t->depth, d_tdepth, P, t->scalars,
                                      t->gimg, t->gdepth);
        if (s == GSRT_OK) s = gsrt_render_splat_depth_grad_async(sc, ubo, GSRT_MODE_COR, k, t->gimg, t->gdepth, t->g_splat, 0);
        if (s == GSRT_OK) s = gsrt_view_stats_add_async(sc, ubo, t->g_splat, t->stats, t->radii);
        if (s == GSRT_OK) s = gsrt_splat_depth_grad_to_model_async(sc, ubo, t->g_splat, t->g_center, t->g_cov, 0);
    } else {
        s = gsrt_render_async(sc, ubo, GSRT_MODE_COR, k, t->rgba, nullptr);
        if (s == GSRT_OK)
            s = gsrt_frame_loss_async(ctx, W, H, t->rgba, d_target, target_channels, d_mask, nullptr, nullptr, P, t->scalars,
                                      t->gimg, nullptr);
        if (s == GSRT_OK) s = gsrt_render_splat_grad_async(sc, ubo, GSRT_MODE_COR, k, t->gimg, t->g_splat, 0);
        if (s == GSRT_OK) s = gsrt_view_stats_add_async(sc, ubo, t->g_splat, t->stats, t->radii);
        if (s == GSRT_OK) s = gsrt_splat_grad_to_model_async(sc, ubo, t->g_splat, t->g_center, t->g_cov, 0);
    }
    if (s == GSRT_OK && t->has_sh) s = gsrt_render_sh_grad_async(sc, ubo, GSRT_MODE_COR, k, t->gimg, t->g_sh, 0);
    if (s == GSRT_OK)
        s = gsrt_model_step_degree_async(ctx, t->n, &raw, &m, &v, &grads, &A, t->sh_degree, nullptr, t->params, t->aabbs, nullptr);
    if (s != GSRT_OK) {
        (void)gsrt_synchronize(ctx);
        return s;
    }
    ++t->step;
    // gsrt_scene_update and gsrt_refit_bvh read their sources on other streams: the step's arrays must be complete
    if ((s = gsrt_synchronize(ctx)) != GSRT_OK) return s;
    if (scalars && hipMemcpy(scalars, t->scalars, sizeof(float) * GSRT_FRAME_LOSS_SCALARS, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(ctx, GSRT_E_DEVICE, name + "scalar download failed");
    if ((s = gsrt_scene_update(sc, t->params, t->aabbs)) != GSRT_OK) return s;
    if ((s = gsrt_refit_bvh(sc, nullptr)) != GSRT_OK) return s;
    if (t->has_sh) s = gsrt_scene_set_sh(sc, raw.sh);
    return s;
}

gsrt_status gsrt_trainer_densify(gsrt_trainer* t, const gsrt_densify_params* P, uint64_t seed, uint32_t* n_out) {
    return gsrt_trainer_densify_screen(t, P, 0.0f, seed, n_out);
}

gsrt_status gsrt_trainer_densify_screen(gsrt_trainer* t, const gsrt_densify_params* P, float max_screen_radius, uint64_t seed,
                                        uint32_t* n_out) {
    if (!t) return GSRT_E_ARG;
    gsrt_ctx* ctx = t->ctx;
    const std::string name = "gsrt_trainer_densify: ";
    if (!P) return fail(ctx, GSRT_E_ARG, name + "params is NULL");
    if (P->reserved[0] || P->reserved[1] || P->reserved[2] || !(P->shrink > 0.0f))
        return fail(ctx, GSRT_E_ARG, name + "bad params (a non-zero reserved word, or shrink not > 0)");
    if (std::isnan(max_screen_radius)) return fail(ctx, GSRT_E_ARG, name + "max_screen_radius is NaN");
    (void)hipSetDevice(ctx->device);
    hipStream_t st = (hipStream_t)gsrt_stream(ctx);
    const int cur = t->cur, oth = 1 - t->cur;
    const gsrt_model_arrays a_in = with_sh_of(t->act[0], t->raw[cur]), a_out = with_sh_of(t->act[1], t->raw[oth]);
    gsrt_status s = gsrt_normal_noise_async(ctx, 6ull * t->n, seed, t->step, t->noise);
    if (s == GSRT_OK) s = gsrt_model_activate_async(ctx, t->n, &t->raw[cur], &a_in, nullptr, nullptr);
    if (s == GSRT_OK)
        s = gsrt_densify_screen_async(ctx, &a_in, t->n, t->stats, t->noise, P, t->radii, max_screen_radius, &a_out, t->origin,
                                      t->cap, t->d_n_out);
    uint32_t rows = 0;
    if (s == GSRT_OK && (hipMemcpyAsync(&rows, t->d_n_out, sizeof rows, hipMemcpyDeviceToHost, st) != hipSuccess ||
                         hipStreamSynchronize(st) != hipSuccess))
        s = fail(ctx, GSRT_E_DEVICE, name + "count download failed");
    if (s != GSRT_OK) return s;
    if (n_out) *n_out = rows;
    if (rows > t->cap)  // the pass wrote nothing
        return fail(ctx, GSRT_E_ARG, name + std::to_string(rows) + " rows needed, the capacity is " + std::to_string(t->cap));
    if (rows == 0) return fail(ctx, GSRT_E_ARG, name + "every Gaussian would be pruned");
    s = gsrt_model_deactivate_async(ctx, rows, &a_out, &t->raw[oth]);
    if (s == GSRT_OK) s = gsrt_model_remap_async(ctx, rows, t->origin, &t->m[cur], &t->m[oth]);
    if (s == GSRT_OK) s = gsrt_model_remap_async(ctx, rows, t->origin, &t->v[cur], &t->v[oth]);
    // the scene is that of the new raw model's activation, as after a step
    if (s == GSRT_OK) s = gsrt_model_activate_async(ctx, rows, &t->raw[oth], &a_out, nullptr, nullptr);
    if (s == GSRT_OK && (hipMemsetAsync(t->stats, 0, sizeof(float) * 2 * (size_t)t->cap, st) != hipSuccess ||
                         hipMemsetAsync(t->radii, 0, sizeof(float) * (size_t)t->cap, st) != hipSuccess))
        s = fail(ctx, GSRT_E_DEVICE, name + "memset failed");
    if (s == GSRT_OK) s = gsrt_synchronize(ctx);
    gsrt_scene* fresh = nullptr;
    if (s == GSRT_OK)
        s = gsrt_scene_from_model(ctx, a_out.center, a_out.rot_rxyz, a_out.scale, a_out.opacity, a_out.sh, rows, &fresh);
    if (s == GSRT_OK) s = gsrt_build_bvh(fresh);
    if (s != GSRT_OK) {
        if (fresh) gsrt_destroy_scene(fresh);
        return s;
    }
    gsrt_destroy_scene(t->scene);
    t->scene = fresh;
    t->cur = oth;
    t->n = rows;
    return GSRT_OK;
}

gsrt_status gsrt_trainer_opacity_reset(gsrt_trainer* t, float max_opacity) {
    if (!t) return GSRT_E_ARG;
    gsrt_ctx* ctx = t->ctx;
    (void)hipSetDevice(ctx->device);
    const int c = t->cur;
    gsrt_status s = gsrt_model_opacity_reset_async(ctx, t->n, t->raw[c].opacity, t->m[c].opacity, t->v[c].opacity, max_opacity);
    if (s != GSRT_OK) return s;  // a refusal: nothing was enqueued
    return scene_follows_raw(t);
}

gsrt_status gsrt_trainer_rebuild_bvh(gsrt_trainer* t) {
    if (!t) return GSRT_E_ARG;
    return gsrt_build_bvh(t->scene);
}

gsrt_status gsrt_trainer_scene(gsrt_trainer* t, gsrt_scene** scene) {
    if (!t || !scene) return GSRT_E_ARG;
    *scene = t->scene;
    return GSRT_OK;
}

gsrt_status gsrt_trainer_info(const gsrt_trainer* t, uint32_t* n, uint32_t* capacity, uint32_t* step) {
    if (!t) return GSRT_E_ARG;
    if (n) *n = t->n;
    if (capacity) *capacity = t->cap;
    if (step) *step = t->step;
    return GSRT_OK;
}

gsrt_status gsrt_trainer_state(gsrt_trainer* t, gsrt_model_arrays* raw, gsrt_model_arrays* m, gsrt_model_arrays* v,
                               gsrt_model_grads* grads, const float** stats) {
    if (!t) return GSRT_E_ARG;
    if (raw) *raw = t->raw[t->cur];
    if (m) *m = t->m[t->cur];
    if (v) *v = t->v[t->cur];
    if (grads) *grads = {t->g_center, t->g_cov, t->g_splat, t->has_sh ? t->g_sh : nullptr, nullptr};
    if (stats) *stats = t->stats;
    return GSRT_OK;
}

gsrt_status gsrt_trainer_radii(gsrt_trainer* t, const float** radii) {
    if (!t || !radii) return GSRT_E_ARG;
    *radii = t->radii;
    return GSRT_OK;
}

gsrt_status gsrt_trainer_set_sh_degree(gsrt_trainer* t, uint32_t sh_degree) {
    if (!t) return GSRT_E_ARG;
    if (sh_degree > 3) return fail(t->ctx, GSRT_E_ARG, "gsrt_trainer_set_sh_degree: sh_degree must be 0..3");
    t->sh_degree = sh_degree;
    return GSRT_OK;
}

gsrt_status gsrt_trainer_sh_degree(const gsrt_trainer* t, uint32_t* sh_degree) {
    if (!t || !sh_degree) return GSRT_E_ARG;
    *sh_degree = t->sh_degree;
    return GSRT_OK;
}

gsrt_status gsrt_trainer_download(gsrt_trainer* t, const gsrt_model_arrays* raw_out, const gsrt_model_arrays* act_out) {
    if (!t) return GSRT_E_ARG;
    gsrt_ctx* ctx = t->ctx;
    const std::string name = "gsrt_trainer_download: ";
    for (const gsrt_model_arrays* o : {raw_out, act_out}) {
        if (!o) continue;
        if (o->features || o->feature_channels) return fail(ctx, GSRT_E_ARG, name + "a trainer's model has no features");
        if (!o->center || !o->rot_rxyz || !o->scale || !o->opacity) return fail(ctx, GSRT_E_ARG, name + "a NULL array");
        if ((o->sh != nullptr) != t->has_sh) return fail(ctx, GSRT_E_ARG, name + "sh is NULL exactly when the model has none");
        ModelField mf[6];
        const uint32_t nf = model_fields(*o, mf);
        for (uint32_t f = 0; f < nf; ++f)
            if (is_device_ptr(o->*mf[f].member)) return fail(ctx, GSRT_E_ARG, name + "the outputs are host arrays");
    }
    (void)hipSetDevice(ctx->device);
    gsrt_status s = gsrt_synchronize(ctx);
    const gsrt_model_arrays a = with_sh_of(t->act[0], t->raw[t->cur]);
    if (s == GSRT_OK && act_out) {
        s = gsrt_model_activate_async(ctx, t->n, &t->raw[t->cur], &a, nullptr, nullptr);
        if (s == GSRT_OK) s = gsrt_synchronize(ctx);
    }
    const auto copy = [&](const gsrt_model_arrays* dst, const gsrt_model_arrays& src) {
        ModelField mf[6];
        const uint32_t nf = model_fields(src, mf);
        for (uint32_t f = 0; f < nf && dst; ++f)
            if (s == GSRT_OK && hipMemcpy(dst->*mf[f].member, src.*mf[f].member, sizeof(float) * mf[f].floats * t->n,
                                          hipMemcpyDeviceToHost) != hipSuccess)
                s = fail(ctx, GSRT_E_DEVICE, name + "download failed");
    };
    copy(raw_out, t->raw[t->cur]);
    copy(act_out, a);
    return s;
}

}  // extern "C"
