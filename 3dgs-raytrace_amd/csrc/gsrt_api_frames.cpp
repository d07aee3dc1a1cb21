// gsrt_api_frames.cpp -- the C ABI's frame entry points (include/gsrt.h): forward frames (colour, depth, features), the
// gradient frames, the projection's backward (gsrt_splat_*grad_to_model) and the camera's gradient (gsrt_pose_grad).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "gsrt_api_util.hpp"

using gsrt::CallArray;
using gsrt::Download;
using gsrt::fail;
using gsrt::finish_blocking;
using gsrt::GradKind;
using gsrt::grow;
using gsrt::is_device_ptr;

extern "C" {

gsrt_status gsrt_comm_fb_render_write(gsrt_ctx* ctx);

// caller: the gradient entry point the frame came through (the only one that may carry its flag), none for every other
static gsrt_status check_render_args(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, GradKind caller = GradKind::none) {
    if (!sc || !ubo) return GSRT_E_ARG;
    if (ubo->width == 0 || ubo->height == 0 || ubo->width > 32768 || ubo->height > 32768)
        return fail(sc->ctx, GSRT_E_ARG, "bad frame size");
    const gsrt::Refusal r = gsrt::frame_refusal(mode, caller, ubo->samples,
                                                {sc->bvh_built, sc->ntri, gsrt_scene_features(sc) != 0, sc->d_sh != nullptr});
    return r.status == GSRT_OK ? GSRT_OK : fail(sc->ctx, r.status, r.msg);
}

static gsrt_status prepare_frame(gsrt_ctx* ctx, const gsrt_ubo* ubo, uint32_t mode, uint32_t feat_channels = 0) {
    const size_t px = (size_t)ubo->width * ubo->height;
    gsrt_status s = grow(ctx, &ctx->d_fb, &ctx->fb_pixels, px * 4);
    if (s != GSRT_OK) return s;
    if (mode & GSRT_FLAG_STATS) {
        s = grow(ctx, &ctx->d_ray_stats, &ctx->ray_stats_pixels, px * 4);
        if (s != GSRT_OK) return s;
    }
    if (mode & GSRT_FLAG_DEPTH) {
        s = grow(ctx, &ctx->d_depth, &ctx->depth_pixels, px);
        if (s != GSRT_OK) return s;
    }
    if (mode & GSRT_FLAG_FEATURES) {
        s = grow(ctx, &ctx->d_feat, &ctx->feat_floats, px * feat_channels);
        if (s != GSRT_OK) return s;
    }
    ctx->last_depth = (mode & GSRT_FLAG_DEPTH) != 0;
    ctx->last_feat = (mode & GSRT_FLAG_FEATURES) != 0;
    ctx->last_w = ubo->width;
    ctx->last_h = ubo->height;
    ctx->last_stats = (mode & GSRT_FLAG_STATS) != 0;
    ctx->last_ref = (mode & 0xffu) == GSRT_MODE_REF;
    return GSRT_OK;
}

// a gradient frame's device buffers (grad_frame_async)
struct GradFrame {
    const float* d_in;   // the upstream gradient image, W x H x channels floats
    float* d_rows;       // the table the render kernel adds to: the zeroed ctx rows, or the caller's table (kFrameFlags)
    uint32_t channels;
    GradKind kind;
    const float* d_in2;  // a kind's second image (FrameFlag::image2_channels: the depth image's gradient), or nullptr
};

// a frame's device outputs: a caller fills the ones its frame has, the others stay nullptr
struct FrameOut {
    float* rgba = nullptr;            // a copy of the frame (the context's framebuffer holds it either way)
    gsrt_raystate* rs = nullptr;      // the per-ray states
    float* depth = nullptr;           // a GSRT_FLAG_DEPTH frame: a copy of ctx->d_depth
    float* feat = nullptr;            // a GSRT_FLAG_FEATURES frame: a copy of ctx->d_feat
    const GradFrame* grad = nullptr;  // a gradient frame's buffers
};

// one frame on the render stream
static gsrt_status render_async(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, const FrameOut& out) {
    float* const d_rgba = out.rgba;
    gsrt_raystate* const d_rs = out.rs;
    gsrt_status s = check_render_args(sc, ubo, mode, out.grad ? out.grad->kind : GradKind::none);
    if (s != GSRT_OK) return s;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    s = prepare_frame(ctx, ubo, mode, sc->feat_channels);
    if (s != GSRT_OK) return s;
    ctx->fb_dump8 = false;
    const gsrt::RenderPlan plan = gsrt::make_plan(*ubo, mode, k, 0, 1);
    gsrt::timing_mark(ctx, 0);
    // pipelined COR frames render into their own buffer while slot streams are chosen (their frames overlap); the
    // ray states are one buffer, so frames that write them stay in order; so are the depth image (GSRT_FLAG_DEPTH) and
    // the feature image (GSRT_FLAG_FEATURES) and a gradient frame's table (a gradient flag got here only with its buffers)
    const bool depth = (mode & GSRT_FLAG_DEPTH) != 0, feat = (mode & GSRT_FLAG_FEATURES) != 0;
    const bool grad = out.grad != nullptr;
    const bool slot = (mode & 0xffu) == GSRT_MODE_COR && !(mode & GSRT_FLAG_STATS) && !d_rs && !depth && !feat && !grad &&
                      gsrt::use_slot_streams(ctx, false);
    if (slot) {
        // the frame goes into one of two alternating buffers (the previous frame's render kernel may still write the
        // other), which becomes the framebuffer view (gsrt_framebuffer)
        const size_t share = (size_t)4 * ubo->width * ubo->height;
        if (ctx->share_floats < share) {
            if ((s = gsrt::sync_all(ctx)) != GSRT_OK) return s;
            ctx->fb_view = nullptr;  // it may point into a buffer freed below; no early return may leave it dangling
            for (int p = 0; p < 2; ++p) {
                (void)hipFree(ctx->d_share[p]);
                ctx->d_share[p] = nullptr;
                ctx->share_pending[p] = false;
            }
            ctx->share_floats = 0;
            for (int p = 0; p < 2; ++p) GSRT_HIP(ctx, hipMalloc(&ctx->d_share[p], sizeof(float) * share));
            ctx->share_floats = share;
        }
        for (int p = 0; p < 2; ++p)
            if (!ctx->ev_share[p]) GSRT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_share[p], kSyncEventFlags));
        const uint32_t p = ctx->share_parity;
        ctx->share_parity ^= 1u;
        gsrt::RenderSync rsy;
        rsy.slot = slot;
        rsy.private_out = true;
        rsy.wait = ctx->share_pending[p] ? ctx->ev_share[p] : nullptr;
        s = gsrt::launch_render(sc, *ubo, plan, ctx->d_share[p], d_rs, &rsy);
        if (s != GSRT_OK) return s;
        ctx->fb_view = ctx->d_share[p];  // the framebuffer of this render (gsrt_framebuffer)
        if (d_rgba && d_rgba != gsrt::framebuffer_of(ctx))
            GSRT_HIP(ctx, hipMemcpyAsync(d_rgba, gsrt::framebuffer_of(ctx), sizeof(float) * 4 * ubo->width * ubo->height,
                                         hipMemcpyDeviceToDevice, ctx->stream));
        GSRT_HIP(ctx, hipEventRecord(ctx->ev_share[p], ctx->stream));  // copies out of d_share[p] issued
        ctx->share_pending[p] = true;
    } else {
        if ((s = gsrt_comm_fb_render_write(ctx)) != GSRT_OK) return s;  // d_fb is also rank 0's unpack target
        gsrt::RenderSync rsy;  // a shared output: frames in order (and render times sampled for use_slot_streams)
        if (depth) rsy.depth = ctx->d_depth;
        if (feat) rsy.feat = ctx->d_feat;
        if (grad) {
            rsy.grad_in = out.grad->d_in;
            rsy.grad_rows = out.grad->d_rows;
            rsy.grad_channels = out.grad->channels;
            rsy.grad_kind = out.grad->kind;
            rsy.grad_depth_in = out.grad->d_in2;
        }
        s = gsrt::launch_render(sc, *ubo, plan, ctx->d_fb, d_rs, d_rs && !depth && !feat && !grad ? nullptr : &rsy);
        if (s != GSRT_OK) return s;
        ctx->fb_view = nullptr;
        if (d_rgba && d_rgba != ctx->d_fb)
            GSRT_HIP(ctx, hipMemcpyAsync(d_rgba, ctx->d_fb, sizeof(float) * 4 * ubo->width * ubo->height,
                                         hipMemcpyDeviceToDevice, ctx->stream));
        if (depth && out.depth && out.depth != ctx->d_depth)
            GSRT_HIP(ctx, hipMemcpyAsync(out.depth, ctx->d_depth, sizeof(float) * ubo->width * ubo->height,
                                         hipMemcpyDeviceToDevice, ctx->stream));
        if (feat && out.feat && out.feat != ctx->d_feat)
            GSRT_HIP(ctx, hipMemcpyAsync(out.feat, ctx->d_feat,
                                         sizeof(float) * ubo->width * ubo->height * sc->feat_channels,
                                         hipMemcpyDeviceToDevice, ctx->stream));
    }
    gsrt::timing_mark(ctx, 3);
    return GSRT_OK;
}

gsrt_status gsrt_render_async(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* d_rgba,
                              gsrt_raystate* d_rs) {
    FrameOut out;
    out.rgba = d_rgba;
    out.rs = d_rs;
    return render_async(sc, ubo, mode, k, out);
}

gsrt_status gsrt_render_depth_async(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* d_rgba,
                                    float* d_depth) {
    FrameOut out;
    out.rgba = d_rgba;
    out.depth = d_depth;
    return render_async(sc, ubo, mode | GSRT_FLAG_DEPTH, k, out);
}

gsrt_status gsrt_render_depth(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* rgba_out,
                              float* depth_out) {
    mode |= GSRT_FLAG_DEPTH;
    gsrt_status s = check_render_args(sc, ubo, mode);
    if (s != GSRT_OK) return s;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    const size_t px = (size_t)ubo->width * ubo->height;
    const bool rgba_dev = is_device_ptr(rgba_out), depth_dev = is_device_ptr(depth_out);
    FrameOut out;
    out.rgba = rgba_dev ? rgba_out : nullptr;
    out.depth = depth_dev ? depth_out : nullptr;
    s = render_async(sc, ubo, mode, k, out);
    return finish_blocking(ctx, s, {{rgba_dev ? nullptr : rgba_out, gsrt::framebuffer_of(ctx), sizeof(float) * 4 * px,
                                     "framebuffer download failed"},
                                    {depth_dev ? nullptr : depth_out, ctx->d_depth, sizeof(float) * px,
                                     "depth download failed"}});
}

const float* gsrt_depth_buffer(gsrt_ctx* ctx) { return ctx && ctx->last_depth ? ctx->d_depth : nullptr; }

gsrt_status gsrt_render_features_async(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* d_rgba,
                                       float* d_feat) {
    FrameOut out;
    out.rgba = d_rgba;
    out.feat = d_feat;
    return render_async(sc, ubo, mode | GSRT_FLAG_FEATURES, k, out);
}

gsrt_status gsrt_render_features(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* rgba_out,
                                 float* feat_out) {
    mode |= GSRT_FLAG_FEATURES;
    gsrt_status s = check_render_args(sc, ubo, mode);
    if (s != GSRT_OK) return s;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    const size_t px = (size_t)ubo->width * ubo->height;
    const bool rgba_dev = is_device_ptr(rgba_out), feat_dev = is_device_ptr(feat_out);
    FrameOut out;
    out.rgba = rgba_dev ? rgba_out : nullptr;
    out.feat = feat_dev ? feat_out : nullptr;
    s = render_async(sc, ubo, mode, k, out);
    return finish_blocking(ctx, s, {{rgba_dev ? nullptr : rgba_out, gsrt::framebuffer_of(ctx), sizeof(float) * 4 * px,
                                     "framebuffer download failed"},
                                    {feat_dev ? nullptr : feat_out, ctx->d_feat, sizeof(float) * px * sc->feat_channels,
                                     "feature image download failed"}});
}

const float* gsrt_feature_buffer(gsrt_ctx* ctx) { return ctx && ctx->last_feat ? ctx->d_feat : nullptr; }

// Gradient frames, each kind by its row F of kFrameFlags. With ctx rows (feature: n x 16 floats, 64-B rows; sh: n x 48,
// 192-B rows in the SH rows' own [rgb][coef] layout: the shapes the render kernel's atomics take) the frame zeroes them, the
// render kernel adds every blended hit's terms to them and a small kernel compacts them into the caller's table (sh:
// transposed into [gauss][coef][rgb]). Without (opacity: n floats in API order; splat: n rows of 8) the render kernel adds to the caller's
// device table itself, zeroed first unless it accumulates, and nothing is compacted. All in order on the render stream: the
// kinds share the ctx's buffers. A kind with a second image (splat_depth: the depth image's gradient) takes it as image2.
static gsrt_status check_grad_args(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, const gsrt::FrameFlag& F,
                                   const float* grad_image, uint32_t channels, const float* grad_table,
                                   const float* grad_image2) {
    if (!sc || !ubo) return GSRT_E_ARG;
    const std::string name = std::string(F.name) + ": ";
    if (!F.image_channels && (channels < 1 || channels > GSRT_MAX_FEATURES))
        return fail(sc->ctx, GSRT_E_ARG, name + "channels must be 1..GSRT_MAX_FEATURES");
    if (!grad_image) return fail(sc->ctx, GSRT_E_ARG, name + "grad_image is NULL");
    if (F.image2_channels && !grad_image2) return fail(sc->ctx, GSRT_E_ARG, name + "grad_depth is NULL");
    if (!grad_table) return fail(sc->ctx, GSRT_E_ARG, name + "grad_table is NULL");
    return check_render_args(sc, ubo, mode, F.kind);
}

static gsrt_status grad_frame_async(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, GradKind kind,
                                    const float* d_image, uint32_t channels, float* d_table, int accumulate,
                                    const float* d_image2 = nullptr) {
    const gsrt::FrameFlag& F = gsrt::grad_flag(kind);
    mode |= F.bit;
    gsrt_status s = check_grad_args(sc, ubo, mode, F, d_image, channels, d_table, d_image2);
    if (s != GSRT_OK) return s;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    if (F.image_channels) channels = F.image_channels;
    if (F.row_floats) {
        const size_t rows = (size_t)F.row_floats * (sc->n ? sc->n : 1);
        if (ctx->grad_rows_floats < rows || !ctx->d_grad_rows) {  // a queued frame may still use the old rows
            if ((s = gsrt::sync_all(ctx)) != GSRT_OK) return s;
            if ((s = grow(ctx, &ctx->d_grad_rows, &ctx->grad_rows_floats, rows)) != GSRT_OK) return s;
        }
        GSRT_HIP(ctx, hipMemsetAsync(ctx->d_grad_rows, 0, sizeof(float) * rows, ctx->stream));
    } else if (!accumulate && sc->n) {
        GSRT_HIP(ctx, hipMemsetAsync(d_table, 0, sizeof(float) * F.table_floats * sc->n, ctx->stream));
    }
    const GradFrame gf{d_image, F.row_floats ? ctx->d_grad_rows : d_table, channels, kind, d_image2};
    FrameOut out;
    out.grad = &gf;
    s = render_async(sc, ubo, mode, k, out);
    if (s != GSRT_OK || !F.row_floats) return s;
    if (kind == GradKind::sh) gsrt::launch_sh_grad_compact(ctx->stream, d_table, ctx->d_grad_rows, sc->n, accumulate != 0);
    else gsrt::launch_grad_compact(ctx->stream, d_table, ctx->d_grad_rows, sc->n, channels, accumulate != 0);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

// a host image and a host table go through the gradient frames' buffers of the ctx (d_grad_in, d_grad_out)
static gsrt_status grad_frame_blocking(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, GradKind kind,
                                       const float* grad_image, uint32_t channels, float* grad_table, int accumulate,
                                       const float* grad_image2 = nullptr) {
    const gsrt::FrameFlag& F = gsrt::grad_flag(kind);
    mode |= F.bit;
    gsrt_status s = check_grad_args(sc, ubo, mode, F, grad_image, channels, grad_table, grad_image2);
    if (s != GSRT_OK) return s;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    const bool in_dev = is_device_ptr(grad_image), out_dev = is_device_ptr(grad_table);
    const bool in2_host = grad_image2 && !is_device_ptr(grad_image2);  // its device copy follows the first image's
    if (accumulate && !out_dev) return fail(ctx, GSRT_E_ARG, std::string(F.name) + ": accumulate needs a device grad_table");
    const size_t in_floats = (size_t)ubo->width * ubo->height * (F.image_channels ? F.image_channels : channels);
    const size_t in2_floats = (size_t)ubo->width * ubo->height * F.image2_channels;
    const size_t in_need = (in_dev ? 0 : in_floats) + (in2_host ? in2_floats : 0);
    const size_t out_floats = (size_t)sc->n * (F.table_floats ? F.table_floats : channels);
    if (in_need && (ctx->grad_in_floats < in_need || !ctx->d_grad_in)) {
        if ((s = gsrt::sync_all(ctx)) != GSRT_OK) return s;
        if ((s = grow(ctx, &ctx->d_grad_in, &ctx->grad_in_floats, in_need)) != GSRT_OK) return s;
    }
    if (!out_dev && (ctx->grad_out_floats < out_floats || !ctx->d_grad_out)) {
        if ((s = gsrt::sync_all(ctx)) != GSRT_OK) return s;
        if ((s = grow(ctx, &ctx->d_grad_out, &ctx->grad_out_floats, out_floats ? out_floats : 1)) != GSRT_OK) return s;
    }
    if (!in_dev)
        GSRT_HIP(ctx, hipMemcpyAsync(ctx->d_grad_in, grad_image, sizeof(float) * in_floats, hipMemcpyHostToDevice, ctx->stream));
    float* const d_in2 = in2_host ? ctx->d_grad_in + (in_dev ? 0 : in_floats) : nullptr;
    if (in2_host)
        GSRT_HIP(ctx, hipMemcpyAsync(d_in2, grad_image2, sizeof(float) * in2_floats, hipMemcpyHostToDevice, ctx->stream));
    s = grad_frame_async(sc, ubo, mode, k, kind, in_dev ? grad_image : ctx->d_grad_in, channels,
                         out_dev ? grad_table : ctx->d_grad_out, accumulate, in2_host ? d_in2 : grad_image2);
    return finish_blocking(ctx, s, {{!out_dev && out_floats ? grad_table : nullptr, ctx->d_grad_out,
                                     sizeof(float) * out_floats, "gradient table download failed"}});
}

gsrt_status gsrt_render_feature_grad_async(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                           const float* d_grad_image, uint32_t channels, float* d_grad_table,
                                           int accumulate) {
    return grad_frame_async(sc, ubo, mode, k, GradKind::feature, d_grad_image, channels, d_grad_table, accumulate);
}
gsrt_status gsrt_render_feature_grad(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                     const float* grad_image, uint32_t channels, float* grad_table, int accumulate) {
    return grad_frame_blocking(sc, ubo, mode, k, GradKind::feature, grad_image, channels, grad_table, accumulate);
}
gsrt_status gsrt_render_sh_grad_async(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                      const float* d_grad_image, float* d_grad_table, int accumulate) {
    return grad_frame_async(sc, ubo, mode, k, GradKind::sh, d_grad_image, 0, d_grad_table, accumulate);
}
gsrt_status gsrt_render_sh_grad(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, const float* grad_image,
                                float* grad_table, int accumulate) {
    return grad_frame_blocking(sc, ubo, mode, k, GradKind::sh, grad_image, 0, grad_table, accumulate);
}
gsrt_status gsrt_render_opacity_grad_async(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                           const float* d_grad_image, float* d_grad_table, int accumulate) {
    return grad_frame_async(sc, ubo, mode, k, GradKind::opacity, d_grad_image, 0, d_grad_table, accumulate);
}
gsrt_status gsrt_render_opacity_grad(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                     const float* grad_image, float* grad_table, int accumulate) {
    return grad_frame_blocking(sc, ubo, mode, k, GradKind::opacity, grad_image, 0, grad_table, accumulate);
}
gsrt_status gsrt_render_splat_grad_async(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                         const float* d_grad_image, float* d_grad_splat, int accumulate) {
    return grad_frame_async(sc, ubo, mode, k, GradKind::splat, d_grad_image, 0, d_grad_splat, accumulate);
}
gsrt_status gsrt_render_splat_grad(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, const float* grad_image,
                                   float* grad_splat, int accumulate) {
    return grad_frame_blocking(sc, ubo, mode, k, GradKind::splat, grad_image, 0, grad_splat, accumulate);
}
gsrt_status gsrt_render_splat_depth_grad_async(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                               const float* d_grad_image, const float* d_grad_depth, float* d_grad_splat,
                                               int accumulate) {
    return grad_frame_async(sc, ubo, mode, k, GradKind::splat_depth, d_grad_image, 0, d_grad_splat, accumulate, d_grad_depth);
}
gsrt_status gsrt_render_splat_depth_grad(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                         const float* grad_image, const float* grad_depth, float* grad_splat,
                                         int accumulate) {
    return grad_frame_blocking(sc, ubo, mode, k, GradKind::splat_depth, grad_image, 0, grad_splat, accumulate, grad_depth);
}

// The projection's backward (k_splat_grad_to_model) on the render stream, behind the splat gradient frame that wrote the
// rows. It reads the scene's current parameter array there as a REF frame's projection does: after the update copies
// the stream has not seen, and an update that retires the array waits for it (serial_pending, serial_reads).
static gsrt_status check_model_grad_args(gsrt_scene* sc, const gsrt_ubo* ubo, const float* rows, const float* gc,
                                         const float* gv, bool depth) {
    if (!sc || !ubo) return GSRT_E_ARG;
    const char* name = depth ? "gsrt_splat_depth_grad_to_model: " : "gsrt_splat_grad_to_model: ";
    if (!rows) return fail(sc->ctx, GSRT_E_ARG, std::string(name) + "grad_splat is NULL");
    if (!gc) return fail(sc->ctx, GSRT_E_ARG, std::string(name) + "grad_center is NULL");
    if (!gv) return fail(sc->ctx, GSRT_E_ARG, std::string(name) + "grad_cov is NULL");
    if (sc->ntri) return fail(sc->ctx, GSRT_E_ARG, std::string(name) + "not for a scene with a triangle mesh");
    if (!sc->bvh_built) return fail(sc->ctx, GSRT_E_STATE, std::string(name) + "before gsrt_build_bvh");
    return GSRT_OK;
}

// depth: the rows are gsrt_render_splat_depth_grad's and slot 6 is chained too (k_splat_grad_to_model<true>)
static gsrt_status model_grad_async(gsrt_scene* sc, const gsrt_ubo* ubo, const float* d_grad_splat, float* d_grad_center,
                                    float* d_grad_cov, int accumulate, bool depth) {
    gsrt_status s = check_model_grad_args(sc, ubo, d_grad_splat, d_grad_center, d_grad_cov, depth);
    if (s != GSRT_OK) return s;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    if (!sc->n) return GSRT_OK;
    if ((s = gsrt::wait_updates(ctx, ctx->stream)) != GSRT_OK) return s;
    ctx->serial_pending = true;
    ctx->serial_reads = true;
    gsrt::launch_splat_grad_to_model(ctx->stream, sc->n, *ubo, sc->d_params, d_grad_splat, d_grad_center, d_grad_cov,
                                     accumulate != 0, depth);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

static gsrt_status model_grad_blocking(gsrt_scene* sc, const gsrt_ubo* ubo, const float* grad_splat, float* grad_center,
                                       float* grad_cov, int accumulate, bool depth) {
    gsrt_status s = check_model_grad_args(sc, ubo, grad_splat, grad_center, grad_cov, depth);
    if (s != GSRT_OK) return s;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    const std::string name = depth ? "gsrt_splat_depth_grad_to_model: " : "gsrt_splat_grad_to_model: ";
    if (accumulate && (!is_device_ptr(grad_center) || !is_device_ptr(grad_cov)))
        return fail(ctx, GSRT_E_ARG, name + "accumulate needs device tables");
    // each table on its own side
    const size_t n = sc->n;
    std::vector<CallArray> list = {{&grad_splat, sizeof(float) * 8 * n, true, false},
                                   {&grad_center, sizeof(float) * 3 * n, false, true},
                                   {&grad_cov, sizeof(float) * 6 * n, false, true}};
    return gsrt::run_staged(ctx, name, list, [&] {
        return model_grad_async(sc, ubo, grad_splat, grad_center, grad_cov, accumulate, depth);
    });
}

gsrt_status gsrt_splat_grad_to_model_async(gsrt_scene* sc, const gsrt_ubo* ubo, const float* d_grad_splat,
                                           float* d_grad_center, float* d_grad_cov, int accumulate) {
    return model_grad_async(sc, ubo, d_grad_splat, d_grad_center, d_grad_cov, accumulate, false);
}
gsrt_status gsrt_splat_grad_to_model(gsrt_scene* sc, const gsrt_ubo* ubo, const float* grad_splat, float* grad_center,
                                     float* grad_cov, int accumulate) {
    return model_grad_blocking(sc, ubo, grad_splat, grad_center, grad_cov, accumulate, false);
}
gsrt_status gsrt_splat_depth_grad_to_model_async(gsrt_scene* sc, const gsrt_ubo* ubo, const float* d_grad_splat,
                                                 float* d_grad_center, float* d_grad_cov, int accumulate) {
    return model_grad_async(sc, ubo, d_grad_splat, d_grad_center, d_grad_cov, accumulate, true);
}
gsrt_status gsrt_splat_depth_grad_to_model(gsrt_scene* sc, const gsrt_ubo* ubo, const float* grad_splat, float* grad_center,
                                           float* grad_cov, int accumulate) {
    return model_grad_blocking(sc, ubo, grad_splat, grad_center, grad_cov, accumulate, true);
}

// ---- per-view statistics with the screen radius (k_view_stats, gsrt_densify.hip) -----------------------------------
// On the render stream behind the gradient frame that wrote the rows, reading the scene's parameters as the chain above.
static gsrt_status check_view_stats_args(gsrt_scene* sc, const gsrt_ubo* ubo, const float* rows, const float* stats) {
    if (!sc || !ubo) return GSRT_E_ARG;
    const std::string name = "gsrt_view_stats_add: ";
    if (!rows || !stats) return fail(sc->ctx, GSRT_E_ARG, name + "grad_splat or stats is NULL");
    if (!ubo->width || !ubo->height) return fail(sc->ctx, GSRT_E_ARG, name + "width and height must be non-zero");
    if (sc->ntri) return fail(sc->ctx, GSRT_E_ARG, name + "not for a scene with a triangle mesh");
    if (!sc->bvh_built) return fail(sc->ctx, GSRT_E_STATE, name + "before gsrt_build_bvh");
    return GSRT_OK;
}

gsrt_status gsrt_view_stats_add_async(gsrt_scene* sc, const gsrt_ubo* ubo, const float* d_grad_splat, float* d_stats,
                                      float* d_radii) {
    gsrt_status s = check_view_stats_args(sc, ubo, d_grad_splat, d_stats);
    if (s != GSRT_OK) return s;
    gsrt_ctx* ctx = sc->ctx;
    if (reinterpret_cast<uintptr_t>(d_grad_splat) % 16u)
        return fail(ctx, GSRT_E_ARG, "gsrt_view_stats_add: grad_splat must be 16-byte aligned on the device");
    (void)hipSetDevice(ctx->device);
    if (!sc->n) return GSRT_OK;
    if (d_radii) {  // the parameters are read only for the radius
        if ((s = gsrt::wait_updates(ctx, ctx->stream)) != GSRT_OK) return s;
        ctx->serial_pending = true;
        ctx->serial_reads = true;
    }
    gsrt::launch_view_stats(ctx->stream, sc->n, *ubo, sc->d_params, d_grad_splat, d_stats, d_radii);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

gsrt_status gsrt_view_stats_add(gsrt_scene* sc, const gsrt_ubo* ubo, const float* grad_splat, float* stats, float* radii) {
    gsrt_status s = check_view_stats_args(sc, ubo, grad_splat, stats);
    if (s != GSRT_OK) return s;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    const size_t n = sc->n;
    std::vector<CallArray> list = {{&grad_splat, sizeof(float) * 8 * n, true, false},
                                   {&stats, sizeof(float) * 2 * n, true, true},
                                   {&radii, sizeof(float) * n, true, true}};
    if (gsrt::call_side(list) == gsrt::Side::mixed)
        return fail(ctx, GSRT_E_ARG, "gsrt_view_stats_add: the arrays must all be host pointers or all be device pointers");
    return gsrt::run_staged(ctx, "gsrt_view_stats_add: ", list,
                            [&] { return gsrt_view_stats_add_async(sc, ubo, grad_splat, stats, radii); });
}

// ---- the camera's gradient (gsrt_pose_grad.hip) -------------------------------------------------------------------
// On the render stream behind the gradient frame that wrote the rows, reading the scene's parameters as the chain above.
static gsrt_status check_pose_grad_args(gsrt_scene* sc, const gsrt_ubo* ubo, const float* rows, const float* out) {
    if (!sc || !ubo) return GSRT_E_ARG;
    const char* name = "gsrt_pose_grad: ";
    if (!rows) return fail(sc->ctx, GSRT_E_ARG, std::string(name) + "grad_splat is NULL");
    if (!out) return fail(sc->ctx, GSRT_E_ARG, std::string(name) + "grad_model_view is NULL");
    if (sc->ntri) return fail(sc->ctx, GSRT_E_ARG, std::string(name) + "not for a scene with a triangle mesh");
    if (!sc->bvh_built) return fail(sc->ctx, GSRT_E_STATE, std::string(name) + "before gsrt_build_bvh");
    return GSRT_OK;
}

// the two kernels on the render stream; the arguments are checked and every pointer is a device pointer (d_out nullptr:
// the workspace's 16 floats, whose address *d_out_used receives)
static gsrt_status pose_grad_enqueue(gsrt_scene* sc, const gsrt_ubo* ubo, const float* d_rows, bool depth, float* d_out,
                                     float** d_out_used = nullptr) {
    gsrt_ctx* ctx = sc->ctx;
    const size_t chunks = gsrt::pose_grad_chunks(sc->n), need = 16 * chunks + 8;
    if (!ctx->d_pose_ws || ctx->pose_ws_doubles < need) {
        GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));  // a queued call may still use the smaller one
        if (gsrt_status s = grow(ctx, &ctx->d_pose_ws, &ctx->pose_ws_doubles, need); s != GSRT_OK) return s;
    }
    // the result's slot stands at the end of the allocation, wherever this call's partials end
    float* const ws_out = reinterpret_cast<float*>(ctx->d_pose_ws + (ctx->pose_ws_doubles - 8));
    if (d_out_used) *d_out_used = d_out ? d_out : ws_out;
    if (gsrt_status s = gsrt::wait_updates(ctx, ctx->stream); s != GSRT_OK) return s;
    ctx->serial_pending = true;
    ctx->serial_reads = true;
    gsrt::launch_pose_grad(ctx->stream, sc->n, *ubo, sc->d_params, d_rows, depth, ctx->d_pose_ws, d_out ? d_out : ws_out);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

gsrt_status gsrt_pose_grad_async(gsrt_scene* sc, const gsrt_ubo* ubo, const float* d_grad_splat, int depth,
                                 float* d_grad_model_view) {
    gsrt_status s = check_pose_grad_args(sc, ubo, d_grad_splat, d_grad_model_view);
    if (s != GSRT_OK) return s;
    (void)hipSetDevice(sc->ctx->device);
    return pose_grad_enqueue(sc, ubo, d_grad_splat, depth != 0, d_grad_model_view);
}

gsrt_status gsrt_pose_grad(gsrt_scene* sc, const gsrt_ubo* ubo, const float* grad_splat, int depth,
                           float grad_model_view[16]) {
    gsrt_status s = check_pose_grad_args(sc, ubo, grad_splat, grad_model_view);
    if (s != GSRT_OK) return s;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    if (is_device_ptr(grad_model_view)) return fail(ctx, GSRT_E_ARG, "gsrt_pose_grad: grad_model_view is a host pointer");
    std::vector<CallArray> list = {{&grad_splat, sizeof(float) * 8 * sc->n, true, false}};
    std::vector<Download> result;  // the workspace's 16 floats
    return gsrt::run_staged(ctx, "gsrt_pose_grad: ", list, [&] {
        float* d_out = nullptr;
        const gsrt_status e = pose_grad_enqueue(sc, ubo, grad_splat, depth != 0, nullptr, &d_out);
        result = {{grad_model_view, d_out, sizeof(float) * 16, "gsrt_pose_grad: download failed"}};
        return e;
    }, &result);
}

gsrt_status gsrt_debug_pose_grad_layout(uint32_t out[2]) {
    if (!out) return GSRT_E_ARG;
    out[0] = gsrt::kPoseChunk;
    out[1] = gsrt::kPoseFinalLanes;
    return GSRT_OK;
}

gsrt_status gsrt_render(gsrt_scene* sc, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* rgba_out,
                        gsrt_raystate* rs_out) {
    gsrt_status s = check_render_args(sc, ubo, mode);
    if (s != GSRT_OK) return s;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    const size_t px = (size_t)ubo->width * ubo->height;
    const bool rgba_dev = is_device_ptr(rgba_out), rs_dev = is_device_ptr(rs_out);
    gsrt_raystate* d_rs = nullptr;
    if (rs_out && !rs_dev) GSRT_HIP(ctx, hipMalloc(&d_rs, sizeof(gsrt_raystate) * px));
    s = gsrt_render_async(sc, ubo, mode, k, rgba_dev ? rgba_out : nullptr, rs_out ? (rs_dev ? rs_out : d_rs) : nullptr);
    void* const tmp = d_rs;  // freed on every path
    return finish_blocking(ctx, s, {{rgba_dev ? nullptr : rgba_out, gsrt::framebuffer_of(ctx), sizeof(float) * 4 * px,
                                     "framebuffer download failed"},
                                    {d_rs ? rs_out : nullptr, d_rs, sizeof(gsrt_raystate) * px, "raystate download failed"}},
                           &tmp);
}

}  // extern "C"
