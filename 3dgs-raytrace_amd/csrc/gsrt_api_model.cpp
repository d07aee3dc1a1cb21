// gsrt_api_model.cpp -- the C ABI's calls on model arrays and images (include/gsrt.h): density statistics and densify,
// the image and frame losses, the optimiser step with activate / deactivate, remap, normal noise and opacity reset.
// Each blocking form describes its arrays in one list (CallArray, gsrt_api_util.hpp) and runs the async body on it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "gsrt_api_util.hpp"

using gsrt::CallArray;
using gsrt::check_adam;
using gsrt::check_call_arrays;
using gsrt::check_model_sets;
using gsrt::Download;
using gsrt::fail;
using gsrt::grow;
using gsrt::is_device_ptr;
using gsrt::model_fields;
using gsrt::model_set_arrays;
using gsrt::ModelField;
using gsrt::run_staged;
using gsrt::Side;

extern "C" {

// ---- adaptive density control (gsrt_densify.hip) ------------------------------------------------------------------
// Everything runs on the render stream: the statistic follows the gradient frame that wrote its rows in stream order.
// The calls work on model arrays, not on a scene, so no scene array is read and no update ordering is involved.
static gsrt_status check_densify_params(gsrt_ctx* ctx, const char* name, const gsrt_densify_params* P) {
    if (!P) return fail(ctx, GSRT_E_ARG, std::string(name) + ": params is NULL");
    if (P->reserved[0] | P->reserved[1] | P->reserved[2])
        return fail(ctx, GSRT_E_ARG, std::string(name) + ": params.reserved must be zero");
    if (!(P->shrink > 0.0f)) return fail(ctx, GSRT_E_ARG, std::string(name) + ": params.shrink must be > 0");
    return GSRT_OK;
}

// the count kernel's workgroup totals and one word for a blocking call's n_out
static gsrt_status densify_workspace(gsrt_ctx* ctx, uint32_t n) {
    const size_t need = (size_t)gsrt::densify_blocks(n) + 1;
    if (ctx->d_densify_ws && ctx->densify_ws_words >= need) return GSRT_OK;
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a queued call may still use the smaller one
    return grow(ctx, &ctx->d_densify_ws, &ctx->densify_ws_words, need);
}

// what both forms of gsrt_density_stats_add refuse first
static gsrt_status check_density_stats_args(gsrt_ctx* ctx, uint32_t n, uint32_t width, uint32_t height,
                                            const float* grad_splat, const float* stats) {
    if (!ctx) return GSRT_E_ARG;
    if (!grad_splat || !stats) return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: a NULL pointer");
    if (!width || !height) return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: width and height must be non-zero");
    if (n > GSRT_MAX_GAUSSIANS) return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: n above GSRT_MAX_GAUSSIANS");
    return GSRT_OK;
}

gsrt_status gsrt_density_stats_add_async(gsrt_ctx* ctx, uint32_t n, uint32_t width, uint32_t height,
                                         const float* d_grad_splat, float* d_stats) {
    if (gsrt_status s = check_density_stats_args(ctx, n, width, height, d_grad_splat, d_stats); s != GSRT_OK) return s;
    if (reinterpret_cast<uintptr_t>(d_grad_splat) % 16u)
        return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: grad_splat must be 16-byte aligned on the device");
    (void)hipSetDevice(ctx->device);
    gsrt::launch_density_stats(ctx->stream, n, width, height, d_grad_splat, d_stats);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

gsrt_status gsrt_density_stats_add(gsrt_ctx* ctx, uint32_t n, uint32_t width, uint32_t height, const float* grad_splat,
                                   float* stats) {
    if (gsrt_status s = check_density_stats_args(ctx, n, width, height, grad_splat, stats); s != GSRT_OK) return s;
    (void)hipSetDevice(ctx->device);
    std::vector<CallArray> list = {{&grad_splat, sizeof(float) * 8 * n, true, false}, {&stats, sizeof(float) * 2 * n, true, true}};
    const Side side = gsrt::call_side(list);
    if (side == Side::mixed)
        return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: the arrays must all be host pointers or all be device pointers");
    if (!n && side == Side::host) return GSRT_OK;  // (device pointers are still held to the async form's alignment)
    return run_staged(ctx, "gsrt_density_stats_add: ", list,
                      [&] { return gsrt_density_stats_add_async(ctx, n, width, height, grad_splat, stats); });
}

// gsrt_densify_count is this with radii nullptr and max_radius 0 (fn: the name the refusals carry)
static gsrt_status densify_count_any(gsrt_ctx* ctx, const char* fn, uint32_t n, const float* scale, const float* opacity,
                                     const float* stats, const gsrt_densify_params* params, const float* radii,
                                     float max_radius, uint32_t* n_out) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = std::string(fn) + ": ";
    if (!n_out || (n && (!scale || !opacity || !stats))) return fail(ctx, GSRT_E_ARG, name + "a NULL pointer");
    if (n > GSRT_MAX_GAUSSIANS) return fail(ctx, GSRT_E_ARG, name + "n above GSRT_MAX_GAUSSIANS");
    if (std::isnan(max_radius)) return fail(ctx, GSRT_E_ARG, name + "max_screen_radius is NaN");
    gsrt_status s = check_densify_params(ctx, fn, params);
    if (s != GSRT_OK) return s;
    *n_out = 0;
    if (!n) return GSRT_OK;
    (void)hipSetDevice(ctx->device);
    if ((s = densify_workspace(ctx, n)) != GSRT_OK) return s;
    // each array on its own side
    std::vector<CallArray> list = {{&scale, sizeof(float) * 3 * n, true, false},
                                   {&opacity, sizeof(float) * n, true, false},
                                   {&stats, sizeof(float) * 2 * n, true, false},
                                   {&radii, sizeof(float) * n, true, false}};
    uint32_t* const d_n = ctx->d_densify_ws + gsrt::densify_blocks(n);
    const std::string what = name + "download failed";
    const std::vector<Download> count = {{n_out, d_n, sizeof(uint32_t), what.c_str()}};
    return run_staged(ctx, name, list, [&]() -> gsrt_status {
        gsrt::launch_densify_count(ctx->stream, n, *params, scale, opacity, stats, radii, max_radius, ctx->d_densify_ws, d_n);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GSRT_E_DEVICE, name + "launch failed");
        return GSRT_OK;
    }, &count);
}

gsrt_status gsrt_densify_count(gsrt_ctx* ctx, uint32_t n, const float* scale, const float* opacity, const float* stats,
                               const gsrt_densify_params* params, uint32_t* n_out) {
    return densify_count_any(ctx, "gsrt_densify_count", n, scale, opacity, stats, params, nullptr, 0.0f, n_out);
}
gsrt_status gsrt_densify_screen_count(gsrt_ctx* ctx, uint32_t n, const float* scale, const float* opacity,
                                      const float* stats, const gsrt_densify_params* params, const float* radii,
                                      float max_screen_radius, uint32_t* n_out) {
    return densify_count_any(ctx, "gsrt_densify_screen_count", n, scale, opacity, stats, params, radii, max_screen_radius,
                             n_out);
}

// what both forms of gsrt_densify refuse before anything is queued
static gsrt_status check_densify_args(gsrt_ctx* ctx, const char* fn, const gsrt_model_arrays* in, uint32_t n,
                                      const float* stats, const float* noise, const gsrt_densify_params* params,
                                      float max_radius, const gsrt_model_arrays* out, const int32_t* origin, uint32_t cap,
                                      const uint32_t* n_out) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = std::string(fn) + ": ";
    if (!in || !out || !n_out) return fail(ctx, GSRT_E_ARG, name + "in, out or n_out is NULL");
    if (gsrt_status s = check_densify_params(ctx, fn, params); s != GSRT_OK) return s;
    if (std::isnan(max_radius)) return fail(ctx, GSRT_E_ARG, name + "max_screen_radius is NaN");
    if (n > GSRT_MAX_GAUSSIANS) return fail(ctx, GSRT_E_ARG, name + "n above GSRT_MAX_GAUSSIANS");
    for (const gsrt_model_arrays* m : {in, out})
        if (m->feature_channels > GSRT_MAX_FEATURES || (m->features == nullptr) != (m->feature_channels == 0))
            return fail(ctx, GSRT_E_ARG, name + "features need 1..GSRT_MAX_FEATURES channels, NULL exactly with 0 channels");
    if ((in->sh == nullptr) != (out->sh == nullptr) || in->feature_channels != out->feature_channels)
        return fail(ctx, GSRT_E_ARG, name + "in and out must agree on sh, features and feature_channels");
    if (n && (!in->center || !in->rot_rxyz || !in->scale || !in->opacity || !stats || !noise))
        return fail(ctx, GSRT_E_ARG, name + "a NULL input array");
    if (n && cap && (!out->center || !out->rot_rxyz || !out->scale || !out->opacity || !origin))
        return fail(ctx, GSRT_E_ARG, name + "a NULL output array");
    ModelField f[6];
    const uint32_t nf = model_fields(*in, f);
    for (uint32_t a = 0; a < nf; ++a)
        if (in->*f[a].member && in->*f[a].member == out->*f[a].member)
            return fail(ctx, GSRT_E_ARG, name + "an out array is the matching in array (the pass is not in place)");
    return GSRT_OK;
}

// both kernels of the pass on the render stream; every pointer is a device pointer and the arguments are checked
static gsrt_status densify_enqueue(gsrt_ctx* ctx, const std::string& name, const gsrt_model_arrays& in, uint32_t n,
                                   const float* d_stats, const float* d_noise, const gsrt_densify_params& P,
                                   const float* d_radii, float max_radius, const gsrt_model_arrays& out, int32_t* d_origin,
                                   uint32_t cap, uint32_t* d_n_out) {
    if ((reinterpret_cast<uintptr_t>(in.sh) | reinterpret_cast<uintptr_t>(out.sh)) % 16u)
        return fail(ctx, GSRT_E_ARG, name + "sh must be 16-byte aligned on the device");
    if (gsrt_status s = densify_workspace(ctx, n); s != GSRT_OK) return s;
    gsrt::launch_densify_count(ctx->stream, n, P, in.scale, in.opacity, d_stats, d_radii, max_radius, ctx->d_densify_ws,
                               d_n_out);
    gsrt::launch_densify_write(ctx->stream, n, P, in, d_stats, d_radii, max_radius, d_noise, out, d_origin, cap,
                               ctx->d_densify_ws, d_n_out);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

// gsrt_densify_async is this with radii nullptr and max_radius 0
static gsrt_status densify_async_any(gsrt_ctx* ctx, const char* fn, const gsrt_model_arrays* in, uint32_t n,
                                     const float* d_stats, const float* d_noise, const gsrt_densify_params* params,
                                     const float* d_radii, float max_radius, const gsrt_model_arrays* out,
                                     int32_t* d_origin, uint32_t cap, uint32_t* d_n_out) {
    gsrt_status s = check_densify_args(ctx, fn, in, n, d_stats, d_noise, params, max_radius, out, d_origin, cap, d_n_out);
    if (s != GSRT_OK) return s;
    (void)hipSetDevice(ctx->device);
    return densify_enqueue(ctx, std::string(fn) + ": ", *in, n, d_stats, d_noise, *params, d_radii, max_radius, *out,
                           d_origin, cap, d_n_out);
}

gsrt_status gsrt_densify_async(gsrt_ctx* ctx, const gsrt_model_arrays* in, uint32_t n, const float* d_stats,
                               const float* d_noise, const gsrt_densify_params* params, const gsrt_model_arrays* out,
                               int32_t* d_origin, uint32_t cap, uint32_t* d_n_out) {
    return densify_async_any(ctx, "gsrt_densify", in, n, d_stats, d_noise, params, nullptr, 0.0f, out, d_origin, cap, d_n_out);
}
gsrt_status gsrt_densify_screen_async(gsrt_ctx* ctx, const gsrt_model_arrays* in, uint32_t n, const float* d_stats,
                                      const float* d_noise, const gsrt_densify_params* params, const float* d_radii,
                                      float max_screen_radius, const gsrt_model_arrays* out, int32_t* d_origin,
                                      uint32_t cap, uint32_t* d_n_out) {
    return densify_async_any(ctx, "gsrt_densify_screen", in, n, d_stats, d_noise, params, d_radii, max_screen_radius, out,
                             d_origin, cap, d_n_out);
}

// gsrt_densify is this with radii nullptr and max_radius 0
static gsrt_status densify_any(gsrt_ctx* ctx, const char* fn, const gsrt_model_arrays* in, uint32_t n, const float* stats,
                               const float* noise, const gsrt_densify_params* params, const float* radii, float max_radius,
                               const gsrt_model_arrays* out, int32_t* origin, uint32_t cap, uint32_t* n_out) {
    gsrt_status s = check_densify_args(ctx, fn, in, n, stats, noise, params, max_radius, out, origin, cap, n_out);
    if (s != GSRT_OK) return s;
    const std::string name = std::string(fn) + ": ";
    *n_out = 0;
    if (!n) return GSRT_OK;
    (void)hipSetDevice(ctx->device);
    // inputs | stats | noise | radii | outputs | origin, all on the host or all on the device (absent arrays take no side)
    gsrt_model_arrays a_in = *in, a_out = *out;
    std::vector<CallArray> list;
    model_set_arrays(list, a_in, n, true, false);
    list.push_back({&stats, sizeof(float) * 2 * n, true, false});
    list.push_back({&noise, sizeof(float) * 6 * n, true, false});
    list.push_back({&radii, sizeof(float) * n, true, false});
    const size_t first_out = list.size();
    model_set_arrays(list, a_out, cap, false, true);
    list.push_back({&origin, sizeof(int32_t) * (size_t)cap, false, true});
    if (gsrt::call_side(list) == Side::mixed)
        return fail(ctx, GSRT_E_ARG, name + "the arrays must all be host pointers or all be device pointers");
    if ((s = densify_workspace(ctx, n)) != GSRT_OK) return s;
    uint32_t* const d_n = ctx->d_densify_ws + gsrt::densify_blocks(n);
    return run_staged(ctx, name, list, [&]() -> gsrt_status {
        gsrt_status e = densify_enqueue(ctx, name, a_in, n, stats, noise, *params, radii, max_radius, a_out, origin, cap, d_n);
        // the count decides what comes back: the stream is drained here for it
        if (e == GSRT_OK && (hipMemcpyAsync(n_out, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                             hipStreamSynchronize(ctx->stream) != hipSuccess))
            e = fail(ctx, GSRT_E_DEVICE, name + "count download failed");
        if (e == GSRT_OK && (*n_out > cap || *n_out > GSRT_MAX_GAUSSIANS))  // the pass wrote nothing
            return fail(ctx, GSRT_E_ARG, name + std::to_string(*n_out) + " output rows needed, cap is " +
                                             std::to_string(cap) + " (at most GSRT_MAX_GAUSSIANS rows)");
        if (e == GSRT_OK && cap)  // only the rows written are downloaded
            for (size_t i = first_out; i < list.size(); ++i) list[i].bytes = list[i].bytes / cap * *n_out;
        return e;
    });
}

gsrt_status gsrt_densify(gsrt_ctx* ctx, const gsrt_model_arrays* in, uint32_t n, const float* stats, const float* noise,
                         const gsrt_densify_params* params, const gsrt_model_arrays* out, int32_t* origin, uint32_t cap,
                         uint32_t* n_out) {
    return densify_any(ctx, "gsrt_densify", in, n, stats, noise, params, nullptr, 0.0f, out, origin, cap, n_out);
}
gsrt_status gsrt_densify_screen(gsrt_ctx* ctx, const gsrt_model_arrays* in, uint32_t n, const float* stats,
                                const float* noise, const gsrt_densify_params* params, const float* radii,
                                float max_screen_radius, const gsrt_model_arrays* out, int32_t* origin, uint32_t cap,
                                uint32_t* n_out) {
    return densify_any(ctx, "gsrt_densify_screen", in, n, stats, noise, params, radii, max_screen_radius, out, origin, cap,
                       n_out);
}

// ---- photometric loss (gsrt_image_loss.hip) -----------------------------------------------------------------------
// On the render stream: behind the frame that wrote rgba and ahead of the gradient frame that reads grad_image. The call
// works on images, not on a scene, so no scene array is read and no update ordering is involved.
gsrt_status gsrt_image_loss_window(float out[11]) {
    if (!out) return GSRT_E_ARG;
    gsrt::image_loss_window(out);
    return GSRT_OK;
}

// what both forms of gsrt_image_loss refuse before anything is queued or written
static gsrt_status check_image_loss_args(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* rgba,
                                         const float* target, uint32_t target_channels, float lambda, const float* out,
                                         const float* grad_image) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = "gsrt_image_loss: ";
    if (!rgba || !target || !out) return fail(ctx, GSRT_E_ARG, name + "rgba, target or out is NULL");
    if (width == 0 || height == 0 || width > 32768 || height > 32768)
        return fail(ctx, GSRT_E_ARG, name + "width and height must be 1..32768");
    if (target_channels != 3 && target_channels != 4) return fail(ctx, GSRT_E_ARG, name + "target_channels must be 3 or 4");
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return fail(ctx, GSRT_E_ARG, name + "lambda must be in [0, 1]");
    if (grad_image) {
        const size_t px = (size_t)width * height;
        const auto overlaps = [&](const float* p, size_t floats) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(grad_image), b = reinterpret_cast<uintptr_t>(p);
            return a < b + sizeof(float) * floats && b < a + sizeof(float) * 4 * px;
        };
        if (overlaps(rgba, 4 * px) || overlaps(target, target_channels * px))
            return fail(ctx, GSRT_E_ARG, name + "grad_image overlaps rgba or target");
    }
    return GSRT_OK;
}

// the call's kernels on the render stream; every pointer is a device pointer (d_out nullptr: the workspace's four
// floats, whose address *d_out_used receives) and the arguments are checked
static gsrt_status image_loss_enqueue(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* d_rgba,
                                      const float* d_target, uint32_t target_channels, float lambda, float* d_out,
                                      float* d_grad, float** d_out_used = nullptr) {
    const uintptr_t wide = reinterpret_cast<uintptr_t>(d_rgba) | reinterpret_cast<uintptr_t>(d_grad) |
                           (target_channels == 4 ? reinterpret_cast<uintptr_t>(d_target) : 0);
    if (wide % 16u)
        return fail(ctx, GSRT_E_ARG, "gsrt_image_loss: rgba, grad_image and a 4-channel target must be 16-byte aligned on the device");
    const size_t px = (size_t)width * height, tiles = gsrt::image_loss_tiles(width, height);
    const size_t need = 3 * tiles + 2 + (d_grad ? (9 * px + 1) / 2 : 0);
    if (!ctx->d_loss_ws || ctx->loss_ws_doubles < need) {
        GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a queued call may still use the smaller one
        if (gsrt_status s = grow(ctx, &ctx->d_loss_ws, &ctx->loss_ws_doubles, need); s != GSRT_OK) return s;
    }
    float* const ws_out = reinterpret_cast<float*>(ctx->d_loss_ws + 3 * tiles);
    if (d_out_used) *d_out_used = d_out ? d_out : ws_out;
    gsrt::launch_image_loss(ctx->stream, width, height, d_rgba, d_target, target_channels, lambda, ctx->d_loss_ws,
                            ws_out + 4, d_out ? d_out : ws_out, d_grad);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

gsrt_status gsrt_image_loss_async(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* d_rgba,
                                  const float* d_target, uint32_t target_channels, float lambda, float* d_out,
                                  float* d_grad_image) {
    gsrt_status s = check_image_loss_args(ctx, width, height, d_rgba, d_target, target_channels, lambda, d_out, d_grad_image);
    if (s != GSRT_OK) return s;
    (void)hipSetDevice(ctx->device);
    return image_loss_enqueue(ctx, width, height, d_rgba, d_target, target_channels, lambda, d_out, d_grad_image);
}

gsrt_status gsrt_image_loss(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* rgba, const float* target,
                            uint32_t target_channels, float lambda, float out[4], float* grad_image) {
    gsrt_status s = check_image_loss_args(ctx, width, height, rgba, target, target_channels, lambda, out, grad_image);
    if (s != GSRT_OK) return s;
    (void)hipSetDevice(ctx->device);
    const size_t px = (size_t)width * height;
    std::vector<CallArray> list = {{&rgba, sizeof(float) * 4 * px, true, false},
                                   {&target, sizeof(float) * target_channels * px, true, false},
                                   {&grad_image, sizeof(float) * 4 * px, false, true}};
    if (gsrt::call_side(list) == Side::mixed)
        return fail(ctx, GSRT_E_ARG, "gsrt_image_loss: rgba, target and grad_image must all be host pointers or all be device pointers");
    if (is_device_ptr(out)) return fail(ctx, GSRT_E_ARG, "gsrt_image_loss: out is a host pointer");
    std::vector<Download> scalars;  // the workspace's four floats
    return run_staged(ctx, "gsrt_image_loss: ", list, [&] {
        float* d_out = nullptr;
        const gsrt_status e = image_loss_enqueue(ctx, width, height, rgba, target, target_channels, lambda, nullptr, grad_image, &d_out);
        scalars = {{out, d_out, sizeof(float) * 4, "gsrt_image_loss: download failed"}};
        return e;
    }, &scalars);
}

// ---- frame loss (gsrt_image_loss.hip): gsrt_image_loss over a background, under a mask, with a depth term ------------
}  // extern "C"

// the refusals of the params struct, also gsrt_trainer_step's under its own name
gsrt_status gsrt::check_frame_loss_params(gsrt_ctx* ctx, const std::string& name, const gsrt_frame_loss_params& P) {
    if (!(P.lambda >= 0.0f && P.lambda <= 1.0f)) return fail(ctx, GSRT_E_ARG, name + "params.lambda must be in [0, 1]");
    if (P.flags & ~GSRT_LOSS_BACKGROUND) return fail(ctx, GSRT_E_ARG, name + "an unknown flag in params.flags");
    if (P.reserved) return fail(ctx, GSRT_E_ARG, name + "params.reserved must be zero");
    if (P.flags & GSRT_LOSS_BACKGROUND)
        for (float b : P.background)
            if (!std::isfinite(b)) return fail(ctx, GSRT_E_ARG, name + "params.background must be finite");
    if (!(P.depth_weight >= 0.0f)) return fail(ctx, GSRT_E_ARG, name + "params.depth_weight is negative or NaN");
    if (!(P.alpha_min > 0.0f && P.alpha_min <= 1.0f)) return fail(ctx, GSRT_E_ARG, name + "params.alpha_min must be in (0, 1]");
    return GSRT_OK;
}

extern "C" {

// what both forms of gsrt_frame_loss refuse before anything is queued or written: the pointers and sizes, around the
// params struct's own refusals
static gsrt_status check_frame_loss_args(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* rgba,
                                         const float* target, uint32_t target_channels, const float* mask,
                                         const float* depth, const float* target_depth, const gsrt_frame_loss_params* P,
                                         const float* out, const float* grad_image, const float* grad_depth) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = "gsrt_frame_loss: ";
    if (!rgba || !target || !out) return fail(ctx, GSRT_E_ARG, name + "rgba, target or out is NULL");
    if (!P) return fail(ctx, GSRT_E_ARG, name + "params is NULL");
    if (width == 0 || height == 0 || width > 32768 || height > 32768)
        return fail(ctx, GSRT_E_ARG, name + "width and height must be 1..32768");
    if (target_channels != 3 && target_channels != 4) return fail(ctx, GSRT_E_ARG, name + "target_channels must be 3 or 4");
    if (gsrt_status s = gsrt::check_frame_loss_params(ctx, name, *P); s != GSRT_OK) return s;
    if (!depth != !target_depth) return fail(ctx, GSRT_E_ARG, name + "depth and target_depth come together or not at all");
    if (grad_depth && (!depth || !grad_image)) return fail(ctx, GSRT_E_ARG, name + "grad_depth needs depth and grad_image");
    const size_t px = (size_t)width * height;
    struct Range {
        const float* p;
        size_t floats;
    };
    const Range in[5] = {{rgba, 4 * px}, {target, target_channels * px}, {mask, px}, {depth, px}, {target_depth, px}};
    const Range outs[3] = {{out, GSRT_FRAME_LOSS_SCALARS}, {grad_image, 4 * px}, {grad_depth, px}};
    const auto overlap = [](const Range& a, const Range& b) {
        const uintptr_t pa = reinterpret_cast<uintptr_t>(a.p), pb = reinterpret_cast<uintptr_t>(b.p);
        return a.p && b.p && pa < pb + sizeof(float) * b.floats && pb < pa + sizeof(float) * a.floats;
    };
    for (int o = 0; o < 3; ++o) {
        for (const Range& r : in)
            if (overlap(outs[o], r)) return fail(ctx, GSRT_E_ARG, name + "an output overlaps an input");
        for (int q = o + 1; q < 3; ++q)
            if (overlap(outs[o], outs[q])) return fail(ctx, GSRT_E_ARG, name + "two outputs overlap");
    }
    return GSRT_OK;
}

// the call's kernels on the render stream; every pointer is a device pointer (d_out nullptr: the workspace's six floats,
// whose address *d_out_used receives) and the arguments are checked
static gsrt_status frame_loss_enqueue(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* d_rgba,
                                      const float* d_target, uint32_t target_channels, const float* d_mask,
                                      const float* d_depth, const float* d_target_depth, const gsrt_frame_loss_params& P,
                                      float* d_out, float* d_grad, float* d_grad_depth, float** d_out_used = nullptr) {
    const uintptr_t wide = reinterpret_cast<uintptr_t>(d_rgba) | reinterpret_cast<uintptr_t>(d_grad) |
                           (target_channels == 4 ? reinterpret_cast<uintptr_t>(d_target) : 0);
    if (wide % 16u)
        return fail(ctx, GSRT_E_ARG, "gsrt_frame_loss: rgba, grad_image and a 4-channel target must be 16-byte aligned on the device");
    const size_t px = (size_t)width * height, tiles = gsrt::image_loss_tiles(width, height);
    const size_t need = 5 * tiles + 3 + (d_grad ? (9 * px + 1) / 2 : 0);
    if (!ctx->d_loss_ws || ctx->loss_ws_doubles < need) {
        GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a queued call may still use the smaller one
        if (gsrt_status s = grow(ctx, &ctx->d_loss_ws, &ctx->loss_ws_doubles, need); s != GSRT_OK) return s;
    }
    float* const ws_out = reinterpret_cast<float*>(ctx->d_loss_ws + 5 * tiles);
    if (d_out_used) *d_out_used = d_out ? d_out : ws_out;
    gsrt::FrameLossArgs A{};
    A.W = width, A.H = height;
    A.rgba = d_rgba, A.target = d_target, A.mask = d_mask, A.depth = d_depth, A.target_depth = d_target_depth;
    A.has_bg = P.flags & GSRT_LOSS_BACKGROUND;
    for (int c = 0; c < 3; ++c) A.bg[c] = A.has_bg ? P.background[c] : 0.0f;
    A.alpha_min = P.alpha_min, A.lambda = P.lambda, A.depth_weight = P.depth_weight;
    gsrt::launch_frame_loss(ctx->stream, A, target_channels, ctx->d_loss_ws, ws_out + GSRT_FRAME_LOSS_SCALARS,
                            d_out ? d_out : ws_out, d_grad, d_grad_depth);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

gsrt_status gsrt_frame_loss_async(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* d_rgba,
                                  const float* d_target, uint32_t target_channels, const float* d_mask,
                                  const float* d_depth, const float* d_target_depth,
                                  const gsrt_frame_loss_params* params, float* d_out, float* d_grad_image,
                                  float* d_grad_depth) {
    gsrt_status s = check_frame_loss_args(ctx, width, height, d_rgba, d_target, target_channels, d_mask, d_depth,
                                          d_target_depth, params, d_out, d_grad_image, d_grad_depth);
    if (s != GSRT_OK) return s;
    (void)hipSetDevice(ctx->device);
    return frame_loss_enqueue(ctx, width, height, d_rgba, d_target, target_channels, d_mask, d_depth, d_target_depth,
                              *params, d_out, d_grad_image, d_grad_depth);
}

gsrt_status gsrt_frame_loss(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* rgba, const float* target,
                            uint32_t target_channels, const float* mask, const float* depth, const float* target_depth,
                            const gsrt_frame_loss_params* params, float out[GSRT_FRAME_LOSS_SCALARS], float* grad_image,
                            float* grad_depth) {
    gsrt_status s = check_frame_loss_args(ctx, width, height, rgba, target, target_channels, mask, depth, target_depth,
                                          params, out, grad_image, grad_depth);
    if (s != GSRT_OK) return s;
    (void)hipSetDevice(ctx->device);
    // rgba | target | mask | depth | target depth | the two gradients (absent ones take no side)
    const size_t px = (size_t)width * height, f = sizeof(float);
    std::vector<CallArray> list = {{&rgba, f * 4 * px, true, false},       {&target, f * target_channels * px, true, false},
                                   {&mask, f * px, true, false},           {&depth, f * px, true, false},
                                   {&target_depth, f * px, true, false},   {&grad_image, f * 4 * px, false, true},
                                   {&grad_depth, f * px, false, true}};
    if (gsrt::call_side(list) == Side::mixed)
        return fail(ctx, GSRT_E_ARG, "gsrt_frame_loss: the images and gradients must all be host pointers or all be device pointers");
    if (is_device_ptr(out)) return fail(ctx, GSRT_E_ARG, "gsrt_frame_loss: out is a host pointer");
    std::vector<Download> scalars;  // the workspace's six floats
    return run_staged(ctx, "gsrt_frame_loss: ", list, [&] {
        float* d_out = nullptr;
        const gsrt_status e = frame_loss_enqueue(ctx, width, height, rgba, target, target_channels, mask, depth, target_depth,
                                                 *params, nullptr, grad_image, grad_depth, &d_out);
        scalars = {{out, d_out, f * GSRT_FRAME_LOSS_SCALARS, "gsrt_frame_loss: download failed"}};
        return e;
    }, &scalars);
}

// ---- the optimiser step (gsrt_model_step.hip) -----------------------------------------------------------------------
// On the render stream, behind the gradient calls that filled the tables. The calls work on model arrays, not on a scene.
static void adam_scalars(const gsrt_adam_params& A, gsrt::AdamScalars& K) {
    const double t = (double)A.step, b1 = (double)A.beta1, b2 = (double)A.beta2;
    const double c1 = 1.0 - std::pow(b1, t);
    const float lr[7] = {A.lr_center, A.lr_rot, A.lr_scale, A.lr_opacity, A.lr_sh_dc, A.lr_sh_rest, A.lr_features};
    K.beta1 = A.beta1;
    K.beta2 = A.beta2;
    K.a1 = (float)(1.0 - b1);
    K.a2 = (float)(1.0 - b2);
    K.c2 = (float)std::sqrt(1.0 - std::pow(b2, t));
    K.eps = A.eps;
    K.frozen = 0;
    for (int i = 0; i < 7; ++i) {
        K.ss[i] = (float)((double)lr[i] / c1);
        if (lr[i] == 0.0f) K.frozen |= 1u << i;
    }
    K.flags = A.flags;
}

gsrt_status gsrt_adam_scalars(const gsrt_adam_params* adam, float out[GSRT_ADAM_SCALARS]) {
    if (!out || check_adam(adam)) return GSRT_E_ARG;
    gsrt::AdamScalars K;
    adam_scalars(*adam, K);
    out[0] = K.a1;
    out[1] = K.a2;
    out[2] = K.c2;
    for (int i = 0; i < 7; ++i) out[3 + i] = K.ss[i];
    return GSRT_OK;
}

// gsrt_model_step (adam != nullptr) and gsrt_model_activate (everything about m, v, grads absent) in one body
static gsrt_status model_step_any(gsrt_ctx* ctx, const char* fn, bool blocking, uint32_t n, const gsrt_model_arrays* raw,
                                  const gsrt_model_arrays* m, const gsrt_model_arrays* v, const gsrt_model_grads* grads,
                                  const gsrt_adam_params* adam, bool step, const gsrt_model_arrays* act,
                                  gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out, float* grad_raw,
                                  uint32_t sh_degree = 3) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = std::string(fn) + ": ";
    if (sh_degree > 3) return fail(ctx, GSRT_E_ARG, name + "sh_degree must be 0..3");
    if (!raw || (step && (!m || !v || !grads || !adam))) return fail(ctx, GSRT_E_ARG, name + "a NULL struct");
    if (step)
        if (const char* why = check_adam(adam)) return fail(ctx, GSRT_E_ARG, name + why);
    if (n > GSRT_MAX_GAUSSIANS) return fail(ctx, GSRT_E_ARG, name + "n above GSRT_MAX_GAUSSIANS");
    if (const char* why = check_model_sets({raw, step ? m : nullptr, step ? v : nullptr, act}, *raw))
        return fail(ctx, GSRT_E_ARG, name + why);
    if (step && ((grads->sh == nullptr) != (raw->sh == nullptr) || (grads->features == nullptr) != (raw->features == nullptr)))
        return fail(ctx, GSRT_E_ARG, name + "grads.sh / grads.features are NULL exactly when the model has none");
    (void)hipSetDevice(ctx->device);
    gsrt_model_arrays r = *raw, mm = step ? *m : gsrt_model_arrays{}, vv = step ? *v : gsrt_model_arrays{};
    gsrt_model_arrays aa = act ? *act : gsrt_model_arrays{};
    gsrt_model_grads gg = step ? *grads : gsrt_model_grads{};
    std::vector<CallArray> list;
    model_set_arrays(list, r, n, true, step);
    if (step) {
        model_set_arrays(list, mm, n, true, true);
        model_set_arrays(list, vv, n, true, true);
        const auto in = [&](const float*& p, size_t floats) { list.push_back({&p, sizeof(float) * floats * n, true, false}); };
        in(gg.center, 3);
        in(gg.cov, 6);
        in(gg.splat, 8);
        if (r.sh) in(gg.sh, 48);
        if (r.features) in(gg.features, r.feature_channels);
    }
    if (act) {
        // act.sh / act.features given as NULL with a model that has them is refused above; every present array is written
        if (n && (!aa.center || !aa.rot_rxyz || !aa.scale || !aa.opacity)) return fail(ctx, GSRT_E_ARG, name + "a NULL array");
        model_set_arrays(list, aa, n, false, true);
    }
    if (params_out) list.push_back({&params_out, sizeof(gsrt_gauss_param) * (size_t)n, false, true});
    if (aabbs_out) list.push_back({&aabbs_out, sizeof(gsrt_aabb) * (size_t)n, false, true});
    if (step && grad_raw) list.push_back({&grad_raw, sizeof(float) * 11 * (size_t)n, false, true});
    if (n && (!r.center || !r.rot_rxyz || !r.scale || !r.opacity ||
              (step && (!mm.center || !mm.rot_rxyz || !mm.scale || !mm.opacity || !vv.center || !vv.rot_rxyz || !vv.scale ||
                        !vv.opacity || !gg.center || !gg.cov || !gg.splat))))
        return fail(ctx, GSRT_E_ARG, name + "a NULL array");
    const int side = check_call_arrays(ctx, name, list, n, {{&aa.sh, &r.sh}, {&aa.features, &r.features}});
    if (side < 0) return GSRT_E_ARG;
    if (!blocking && side == 0 && n) return fail(ctx, GSRT_E_ARG, name + "the async form takes device pointers only");
    gsrt::AdamScalars K{};
    if (step) adam_scalars(*adam, K);
    const auto run = [&]() -> gsrt_status {
        gsrt::launch_model_step(ctx->stream, n, step ? &K : nullptr, r, &mm, &vv, &gg, aa, params_out, aabbs_out, grad_raw,
                                sh_degree);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GSRT_E_DEVICE, name + "launch failed");
        return GSRT_OK;
    };
    if (!n) return GSRT_OK;
    return blocking ? run_staged(ctx, name, list, run) : run();
}

gsrt_status gsrt_model_step(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw, const gsrt_model_arrays* m,
                            const gsrt_model_arrays* v, const gsrt_model_grads* grads, const gsrt_adam_params* adam,
                            const gsrt_model_arrays* act, gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out,
                            float* grad_raw) {
    return model_step_any(ctx, "gsrt_model_step", true, n, raw, m, v, grads, adam, true, act, params_out, aabbs_out, grad_raw);
}
gsrt_status gsrt_model_step_async(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw, const gsrt_model_arrays* m,
                                  const gsrt_model_arrays* v, const gsrt_model_grads* grads, const gsrt_adam_params* adam,
                                  const gsrt_model_arrays* act, gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out,
                                  float* grad_raw) {
    return model_step_any(ctx, "gsrt_model_step", false, n, raw, m, v, grads, adam, true, act, params_out, aabbs_out, grad_raw);
}
gsrt_status gsrt_model_step_degree(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw, const gsrt_model_arrays* m,
                                   const gsrt_model_arrays* v, const gsrt_model_grads* grads, const gsrt_adam_params* adam,
                                   uint32_t sh_degree, const gsrt_model_arrays* act, gsrt_gauss_param* params_out,
                                   gsrt_aabb* aabbs_out, float* grad_raw) {
    return model_step_any(ctx, "gsrt_model_step_degree", true, n, raw, m, v, grads, adam, true, act, params_out, aabbs_out,
                          grad_raw, sh_degree);
}
gsrt_status gsrt_model_step_degree_async(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw,
                                         const gsrt_model_arrays* m, const gsrt_model_arrays* v,
                                         const gsrt_model_grads* grads, const gsrt_adam_params* adam, uint32_t sh_degree,
                                         const gsrt_model_arrays* act, gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out,
                                         float* grad_raw) {
    return model_step_any(ctx, "gsrt_model_step_degree", false, n, raw, m, v, grads, adam, true, act, params_out, aabbs_out,
                          grad_raw, sh_degree);
}
gsrt_status gsrt_model_activate(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw, const gsrt_model_arrays* act,
                                gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out) {
    return model_step_any(ctx, "gsrt_model_activate", true, n, raw, nullptr, nullptr, nullptr, nullptr, false, act, params_out,
                          aabbs_out, nullptr);
}
gsrt_status gsrt_model_activate_async(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw, const gsrt_model_arrays* act,
                                      gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out) {
    return model_step_any(ctx, "gsrt_model_activate", false, n, raw, nullptr, nullptr, nullptr, nullptr, false, act, params_out,
                          aabbs_out, nullptr);
}

static gsrt_status model_deactivate_any(gsrt_ctx* ctx, bool blocking, uint32_t n, const gsrt_model_arrays* act,
                                        const gsrt_model_arrays* raw) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = "gsrt_model_deactivate: ";
    if (!act || !raw) return fail(ctx, GSRT_E_ARG, name + "a NULL struct");
    if (n > GSRT_MAX_GAUSSIANS) return fail(ctx, GSRT_E_ARG, name + "n above GSRT_MAX_GAUSSIANS");
    if (const char* why = check_model_sets({act, raw}, *act)) return fail(ctx, GSRT_E_ARG, name + why);
    (void)hipSetDevice(ctx->device);
    gsrt_model_arrays a = *act, r = *raw;
    if (n && (!a.center || !a.rot_rxyz || !a.scale || !a.opacity || !r.center || !r.rot_rxyz || !r.scale || !r.opacity))
        return fail(ctx, GSRT_E_ARG, name + "a NULL array");
    std::vector<CallArray> list;
    model_set_arrays(list, a, n, true, false);
    model_set_arrays(list, r, n, false, true);
    const int side = check_call_arrays(ctx, name, list, n, {{&a.sh, &r.sh}, {&a.features, &r.features}});
    if (side < 0) return GSRT_E_ARG;
    if (!blocking && side == 0 && n) return fail(ctx, GSRT_E_ARG, name + "the async form takes device pointers only");
    const auto run = [&]() -> gsrt_status {
        gsrt::launch_model_deactivate(ctx->stream, n, a, r);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GSRT_E_DEVICE, name + "launch failed");
        return GSRT_OK;
    };
    if (!n) return GSRT_OK;
    return blocking ? run_staged(ctx, name, list, run) : run();
}
gsrt_status gsrt_model_deactivate(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* act, const gsrt_model_arrays* raw) {
    return model_deactivate_any(ctx, true, n, act, raw);
}
gsrt_status gsrt_model_deactivate_async(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* act,
                                        const gsrt_model_arrays* raw) {
    return model_deactivate_any(ctx, false, n, act, raw);
}

// gsrt_model_remap: the call is not told how many rows `in` has. With a host origin it reads the count off it (the
// largest entry + 1), which sizes the staging and the overlap check; a device origin is not read on the host, and only
// the first row of each `in` array takes part in the overlap check then.
static gsrt_status model_remap_any(gsrt_ctx* ctx, bool blocking, uint32_t n_out, const int32_t* origin,
                                   const gsrt_model_arrays* in, const gsrt_model_arrays* out) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = "gsrt_model_remap: ";
    if (!in || !out) return fail(ctx, GSRT_E_ARG, name + "a NULL struct");
    if (n_out > GSRT_MAX_GAUSSIANS) return fail(ctx, GSRT_E_ARG, name + "n_out above GSRT_MAX_GAUSSIANS");
    if (const char* why = check_model_sets({in, out}, *in)) return fail(ctx, GSRT_E_ARG, name + why);
    (void)hipSetDevice(ctx->device);
    gsrt_model_arrays a = *in, r = *out;
    if (n_out && (!origin || !a.center || !a.rot_rxyz || !a.scale || !a.opacity || !r.center || !r.rot_rxyz || !r.scale ||
                  !r.opacity))
        return fail(ctx, GSRT_E_ARG, name + "a NULL array");
    if (!n_out) return GSRT_OK;
    size_t n_in = 1;
    if (!is_device_ptr(origin)) {
        int64_t rows = 0;
        for (uint32_t i = 0; i < n_out; ++i) rows = std::max<int64_t>(rows, (int64_t)origin[i] + 1);
        n_in = (size_t)rows;
    }
    std::vector<CallArray> list;
    model_set_arrays(list, a, n_in, true, false);
    model_set_arrays(list, r, n_out, false, true);
    list.push_back({&origin, sizeof(int32_t) * (size_t)n_out, true, false});
    const int side = check_call_arrays(ctx, name, list, n_out, {});
    if (side < 0) return GSRT_E_ARG;
    if (!blocking && side == 0) return fail(ctx, GSRT_E_ARG, name + "the async form takes device pointers only");
    const auto run = [&]() -> gsrt_status {
        gsrt::launch_model_remap(ctx->stream, n_out, origin, a, r);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GSRT_E_DEVICE, name + "launch failed");
        return GSRT_OK;
    };
    return blocking ? run_staged(ctx, name, list, run) : run();
}
gsrt_status gsrt_model_remap(gsrt_ctx* ctx, uint32_t n_out, const int32_t* origin, const gsrt_model_arrays* in,
                             const gsrt_model_arrays* out) {
    return model_remap_any(ctx, true, n_out, origin, in, out);
}
gsrt_status gsrt_model_remap_async(gsrt_ctx* ctx, uint32_t n_out, const int32_t* d_origin, const gsrt_model_arrays* in,
                                   const gsrt_model_arrays* out) {
    return model_remap_any(ctx, false, n_out, d_origin, in, out);
}

// ---- normal noise (gsrt_rng.hip) ----------------------------------------------------------------------------------
gsrt_status gsrt_normal_noise_async(gsrt_ctx* ctx, uint64_t count, uint64_t seed, uint32_t stream_id, float* d_out) {
    if (!ctx) return GSRT_E_ARG;
    if (!count) return GSRT_OK;
    if (!d_out) return fail(ctx, GSRT_E_ARG, "gsrt_normal_noise: out is NULL");
    if (!is_device_ptr(d_out)) return fail(ctx, GSRT_E_ARG, "gsrt_normal_noise: the async form takes a device pointer only");
    if (reinterpret_cast<uintptr_t>(d_out) % 4u) return fail(ctx, GSRT_E_ARG, "gsrt_normal_noise: out is not 4-byte aligned");
    (void)hipSetDevice(ctx->device);
    gsrt::launch_normal_noise(ctx->stream, count, seed, stream_id, d_out);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}
gsrt_status gsrt_normal_noise(gsrt_ctx* ctx, uint64_t count, uint64_t seed, uint32_t stream_id, float* out) {
    if (!ctx) return GSRT_E_ARG;
    if (!count) return GSRT_OK;
    if (!out) return fail(ctx, GSRT_E_ARG, "gsrt_normal_noise: out is NULL");
    (void)hipSetDevice(ctx->device);
    std::vector<CallArray> list = {{&out, sizeof(float) * count, false, true}};
    return run_staged(ctx, "gsrt_normal_noise: ", list, [&] { return gsrt_normal_noise_async(ctx, count, seed, stream_id, out); });
}

static gsrt_status opacity_reset_any(gsrt_ctx* ctx, bool blocking, uint32_t n, float* logit, float* m, float* v,
                                     float max_opacity) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = "gsrt_model_opacity_reset: ";
    if (!(max_opacity > 0.0f && max_opacity < 1.0f)) return fail(ctx, GSRT_E_ARG, name + "max_opacity must be in (0, 1)");
    if (n > GSRT_MAX_GAUSSIANS) return fail(ctx, GSRT_E_ARG, name + "n above GSRT_MAX_GAUSSIANS");
    (void)hipSetDevice(ctx->device);
    std::vector<CallArray> list = {{&logit, sizeof(float) * (size_t)n, true, true},
                                   {&m, sizeof(float) * (size_t)n, false, true},
                                   {&v, sizeof(float) * (size_t)n, false, true}};
    const int side = check_call_arrays(ctx, name, list, n, {});
    if (side < 0) return GSRT_E_ARG;
    if (!blocking && side == 0 && n) return fail(ctx, GSRT_E_ARG, name + "the async form takes device pointers only");
    const float limit = (float)std::log((double)max_opacity / (1.0 - (double)max_opacity));
    const auto run = [&]() -> gsrt_status {
        gsrt::launch_opacity_reset(ctx->stream, n, limit, logit, m, v);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GSRT_E_DEVICE, name + "launch failed");
        return GSRT_OK;
    };
    if (!n) return GSRT_OK;
    return blocking ? run_staged(ctx, name, list, run) : run();
}
gsrt_status gsrt_model_opacity_reset(gsrt_ctx* ctx, uint32_t n, float* logit_opacity, float* m_opacity, float* v_opacity,
                                     float max_opacity) {
    return opacity_reset_any(ctx, true, n, logit_opacity, m_opacity, v_opacity, max_opacity);
}
gsrt_status gsrt_model_opacity_reset_async(gsrt_ctx* ctx, uint32_t n, float* d_logit_opacity, float* d_m_opacity,
                                           float* d_v_opacity, float max_opacity) {
    return opacity_reset_any(ctx, false, n, d_logit_opacity, d_m_opacity, d_v_opacity, max_opacity);
}

}  // extern "C"
