// gsrt_api.cpp -- the C ABI (include/gsrt.h): context, scene upload, LBVH, render, stats.
#include <algorithm>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <new>

#include "gsrt_internal.hpp"

using gsrt::fail;
using gsrt::GradKind;

namespace {

bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

template <class T>
gsrt_status grow(gsrt_ctx* ctx, T** p, size_t* have, size_t need) {
    if (*have >= need && *p) return GSRT_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    if (hipMalloc(p, sizeof(T) * need) != hipSuccess) return fail(ctx, GSRT_E_OOM, "device allocation failed");
    *have = need;
    return GSRT_OK;
}

// a blocking call's device copies of host arrays: regions of whole 16-byte units of one block, handed out in order
struct Staging {
    char* base = nullptr;
    size_t used = 0;
    static size_t unit(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
    template <class T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base + used);
        used += unit(sizeof(T) * count);
        return p;
    }
};

gsrt_status upload_common(gsrt_ctx* ctx, uint32_t n, const float* sh, gsrt_scene* sc) {
    sc->d_buf[0][0] = sc->d_params;
    sc->d_buf[1][0] = sc->d_aabbs;
    if (gsrt_status s = gsrt::lbvh_alloc(sc); s != GSRT_OK) return s;  // the BVH's buffers: a build allocates nothing
    GSRT_HIP(ctx, hipMalloc(&sc->d_flags, sizeof(uint32_t) * 4));
    GSRT_HIP(ctx, hipMemset(sc->d_flags, 0, sizeof(uint32_t) * 4));
    GSRT_HIP(ctx, hipMalloc(&sc->d_recs[0], sizeof(gsrt::SplatRec) * (n ? n : 1)));  // [1]: on the first COR frame
    GSRT_HIP(ctx, hipMalloc(&sc->d_keyed[0], sizeof(uint32_t) * ((n + 31) / 32 + 1)));
    GSRT_HIP(ctx, hipMemset(sc->d_keyed[0], 0xFF, sizeof(uint32_t) * ((n + 31) / 32 + 1)));
    if (sh) {
        // API layout [gauss][coef 16][rgb] -> device layout [gauss][rgb][coef 16]: one colour channel is 64
        // contiguous bytes, read as four 16-B LDS broadcasts by the blend loop. Word 0 of a channel holds the
        // ray-independent part of the colour, (s_0 Y_0) + 0.5 (Y_0 = 0.28209479 the constant DC basis), which
        // the shading loop's fma chain over k = 1..15 starts from (the COR colour's order, oracle sh_color)
        std::vector<float> t(48ull * n);
        for (size_t i = 0; i < n; ++i)
            for (int c = 0; c < 3; ++c) {
                t[48 * i + 16 * c] = sh[48 * i + c] * gsrt::kShY0 + 0.5f;
                for (int k = 1; k < 16; ++k) t[48 * i + 16 * c + k] = sh[48 * i + 3 * k + c];
            }
        GSRT_HIP(ctx, hipMalloc(&sc->d_sh, sizeof(float) * 48ull * n));
        GSRT_HIP(ctx, hipMemcpy(sc->d_sh, t.data(), sizeof(float) * 48ull * n, hipMemcpyHostToDevice));
    }
    return GSRT_OK;
}

}  // namespace

namespace gsrt {
gsrt_status sync_all(gsrt_ctx* ctx) {
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->ustream) GSRT_HIP(ctx, hipStreamSynchronize(ctx->ustream));
    for (uint32_t j = 0; j < kStreamSlots; ++j)
        for (hipStream_t p : {ctx->prep_hi[j], ctx->prep_lo[j]})
            if (p) GSRT_HIP(ctx, hipStreamSynchronize(p));
    return GSRT_OK;
}

gsrt_status wait_updates(gsrt_ctx* ctx, hipStream_t s) {
    if (!ctx->copy_unseen) return GSRT_OK;
    const hipStream_t streams[5] = {ctx->prep_hi[0], ctx->prep_hi[1], ctx->prep_lo[0], ctx->prep_lo[1], ctx->stream};
    for (uint32_t i = 0; i < 5; ++i)
        if (streams[i] == s && ((ctx->copy_unseen >> i) & 1u)) {
            GSRT_HIP(ctx, hipStreamWaitEvent(s, ctx->ev_copied, 0));
            ctx->copy_unseen &= ~(1u << i);
        }
    return GSRT_OK;
}

gsrt_status check_error_word(gsrt_ctx* ctx) {
    gsrt_status s = sync_all(ctx);
    if (s != GSRT_OK) return s;
    unsigned long long err = 0;
    GSRT_HIP(ctx, hipMemcpy(&err, ctx->d_counters + kErrWord, sizeof err, hipMemcpyDeviceToHost));
    if (!err) return GSRT_OK;
    // cleared on the render stream and waited for here, inside the sync window: the ctx's streams are non-blocking,
    // so a null-stream memset would not be ordered against the next frame's kernels (which atomicOr this word)
    GSRT_HIP(ctx, hipMemsetAsync(ctx->d_counters + kErrWord, 0, sizeof err, ctx->stream));
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return fail(ctx, GSRT_E_DEVICE, "render: traversal stack overflow (a frame since the last check is incomplete)");
}

void timing_mark(gsrt_ctx* ctx, int which, hipStream_t s) {
    if (ctx->timing_n >= ctx->timing_cap) return;
    const bool rec = ctx->timing_frame % ctx->timing_stride == 0;  // this frame is a sampled one
    if (rec) {
        if (!(ctx->timing_kernel_only && (which == 0 || which == 3)))
            (void)hipEventRecord(ctx->events[kTimingEvents * ctx->timing_n + which], s ? s : ctx->stream);
        if (which == 0) ctx->timing_ex[ctx->timing_n] = 0;
        if (which == 4) ctx->timing_ex[ctx->timing_n] = 1;
    }
    if (which == 3) {
        if (rec) ++ctx->timing_n;
        ++ctx->timing_frame;
    }
}
}  // namespace gsrt

extern "C" {

int gsrt_abi_version(void) { return GSRT_ABI_VERSION; }

const char* gsrt_status_string(gsrt_status s) {
    switch (s) {
        case GSRT_OK: return "ok";
        case GSRT_E_ARG: return "invalid argument";
        case GSRT_E_OOM: return "out of memory";
        case GSRT_E_DEVICE: return "device error";
        case GSRT_E_IO: return "i/o error";
        case GSRT_E_STATE: return "invalid state";
        case GSRT_E_COMM: return "communication error";
    }
    return "unknown";
}

gsrt_status gsrt_create(gsrt_ctx** out, int device) {
    if (!out) return GSRT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        return GSRT_E_DEVICE;
    }
    gsrt_ctx* ctx = new (std::nothrow) gsrt_ctx();
    if (!ctx) return GSRT_E_OOM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return GSRT_E_DEVICE;
    }
    // the prep streams in two priority classes (kPrioLowAboveUs): pstream / fstream start at the highest
    // (test switch GSRT_DEBUG_PREP_PRIORITY=0: always the lowest, 1: always the highest, 2: switch every frame)
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    const char* pe = std::getenv("GSRT_DEBUG_PREP_PRIORITY");
    ctx->prep_high = !(pe && pe[0] == '0');
    bool ev_ok = true;
    for (uint32_t j = 0; j < kStreamSlots; ++j)
        ev_ok = ev_ok && hipStreamCreateWithPriority(&ctx->prep_hi[j], hipStreamNonBlocking, prio_greatest) == hipSuccess &&
                hipStreamCreateWithPriority(&ctx->prep_lo[j], hipStreamNonBlocking, prio_least) == hipSuccess &&
                hipEventCreateWithFlags(&ctx->ev_hop[j], kSyncEventFlags) == hipSuccess &&
                hipEventCreateWithFlags(&ctx->ev_side[j], kSyncEventFlags) == hipSuccess;
    // The update and comm streams are created here too, so that the context's streams always come in one order:
    // render (default priority), prep H / L / H / L, update (H), comm (default); RCCL's own stream follows at
    // gsrt_comm_init. A hardware queue of the process holds streams of one priority only, so the render and comm streams
    // are the context's only default-priority ones and share no queue with a prep or update stream
    // (profiles/r06/queue_map.txt). Test switch GSRT_DEBUG_LAZY_STREAMS=1: both created when first used, at the
    // default priority (the round-5 order)
    const char* lz = std::getenv("GSRT_DEBUG_LAZY_STREAMS");
    if (ev_ok && !(lz && lz[0] == '1'))
        ev_ok = hipStreamCreateWithPriority(&ctx->ustream, hipStreamNonBlocking, prio_greatest) == hipSuccess &&
                hipEventCreateWithFlags(&ctx->ev_copied, kSyncEventFlags) == hipSuccess &&
                hipStreamCreateWithFlags(&ctx->cstream, hipStreamNonBlocking) == hipSuccess;
    if (ev_ok) {
        hipStream_t* set = ctx->prep_high ? ctx->prep_hi : ctx->prep_lo;
        ctx->pstream = set[0];
        ctx->fstream = set[1];
    }
    ev_ok = ev_ok &&
                 hipEventCreateWithFlags(&ctx->ev_fit, kSyncEventFlags) == hipSuccess &&
                 hipEventCreateWithFlags(&ctx->ev_front, kSyncEventFlags) == hipSuccess &&
                 hipEventCreateWithFlags(&ctx->ev_lists, kSyncEventFlags) == hipSuccess &&
                 hipEventCreateWithFlags(&ctx->ev_main, kSyncEventFlags) == hipSuccess &&
                 hipEventCreateWithFlags(&ctx->ev_serial, kSyncEventFlags) == hipSuccess;
    for (FrameSlot& S : ctx->slot)
        ev_ok = ev_ok && hipEventCreateWithFlags(&S.prepared, kSyncEventFlags) == hipSuccess &&
                hipEventCreateWithFlags(&S.rendered, kSyncEventFlags) == hipSuccess &&
                hipEventCreateWithFlags(&S.t0, kTimingEventFlags) == hipSuccess &&
                hipEventCreateWithFlags(&S.t1, kTimingEventFlags) == hipSuccess;
    if (!ev_ok) {
        gsrt_destroy(ctx);
        return GSRT_E_DEVICE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        ctx->num_cus = prop.multiProcessorCount;
    if (hipMalloc(&ctx->d_counters, sizeof(unsigned long long) * gsrt::kCounters) != hipSuccess ||
        hipMalloc(&ctx->d_tile_counter, sizeof(uint32_t) * 4) != hipSuccess ||
        hipMalloc(&ctx->d_lut, sizeof(float) * 512) != hipSuccess) {
        gsrt_destroy(ctx);
        return GSRT_E_OOM;
    }
    float lut[512];
    gsrt::exp_lut(lut);
    if (hipMemcpy(ctx->d_lut, lut, sizeof lut, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(ctx->d_counters, 0, sizeof(unsigned long long) * gsrt::kCounters) != hipSuccess) {
        gsrt_destroy(ctx);
        return GSRT_E_DEVICE;
    }
    *out = ctx;
    return GSRT_OK;
}

void gsrt_comm_destroy_internal(gsrt_ctx* ctx);
hipStream_t gsrt_comm_stream_internal(gsrt_ctx* ctx);
gsrt_status gsrt_comm_sync_internal(gsrt_ctx* ctx);
gsrt_status gsrt_comm_fb_render_write(gsrt_ctx* ctx);

void gsrt_destroy(gsrt_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    gsrt_comm_destroy_internal(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (uint32_t j = 0; j < kStreamSlots; ++j)
        for (hipStream_t p : {ctx->prep_hi[j], ctx->prep_lo[j]})
            if (p) (void)hipStreamSynchronize(p);
    if (ctx->ustream) {
        (void)hipStreamSynchronize(ctx->ustream);
        (void)hipStreamDestroy(ctx->ustream);
    }
    if (ctx->ev_copied) (void)hipEventDestroy(ctx->ev_copied);
    if (ctx->cstream) (void)hipStreamDestroy(ctx->cstream);  // (the communicator, which used it, is gone)
    (void)hipFree(ctx->d_fb);
    for (int p = 0; p < 2; ++p) {
        (void)hipFree(ctx->d_share[p]);
        if (ctx->ev_share[p]) (void)hipEventDestroy(ctx->ev_share[p]);
    }
    (void)hipFree(ctx->d_ray_stats);
    (void)hipFree(ctx->d_depth);
    (void)hipFree(ctx->d_feat);
    (void)hipFree(ctx->d_grad_rows);
    (void)hipFree(ctx->d_grad_in);
    (void)hipFree(ctx->d_grad_out);
    (void)hipFree(ctx->d_densify_ws);
    (void)hipFree(ctx->d_loss_ws);
    (void)hipFree(ctx->d_pose_ws);
    (void)hipFree(ctx->d_counters);
    (void)hipFree(ctx->d_tile_counter);
    (void)hipFree(ctx->d_lut);
    (void)hipFree(ctx->d_tri_t);
    for (FrameSlot& S : ctx->slot) {
        (void)hipFree(S.d_lists);
        (void)hipFree(S.d_list_hdr);
        (void)hipFree(S.d_glist);
        (void)hipFree(S.d_ghdr);
        (void)hipFree(S.d_frontier);
        if (S.prepared) (void)hipEventDestroy(S.prepared);
        if (S.rendered) (void)hipEventDestroy(S.rendered);
        if (S.t0) (void)hipEventDestroy(S.t0);
        if (S.t1) (void)hipEventDestroy(S.t1);
    }
    (void)hipFree(ctx->d_group_order);
    (void)hipFree(ctx->d_run_order);
    for (uint32_t j = 0; j < kSlots; ++j) (void)hipFree(ctx->d_tile_cost[j]);
    for (hipEvent_t e : ctx->events) (void)hipEventDestroy(e);
    if (ctx->ev_main) (void)hipEventDestroy(ctx->ev_main);
    if (ctx->ev_serial) (void)hipEventDestroy(ctx->ev_serial);
    if (ctx->ev_fit) (void)hipEventDestroy(ctx->ev_fit);
    if (ctx->ev_front) (void)hipEventDestroy(ctx->ev_front);
    if (ctx->ev_lists) (void)hipEventDestroy(ctx->ev_lists);
    for (uint32_t j = 0; j < kStreamSlots; ++j) {
        if (ctx->ev_hop[j]) (void)hipEventDestroy(ctx->ev_hop[j]);
        if (ctx->ev_side[j]) (void)hipEventDestroy(ctx->ev_side[j]);
        if (ctx->prep_hi[j]) (void)hipStreamDestroy(ctx->prep_hi[j]);
        if (ctx->prep_lo[j]) (void)hipStreamDestroy(ctx->prep_lo[j]);
    }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* gsrt_last_error(const gsrt_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

gsrt_status gsrt_synchronize(gsrt_ctx* ctx) {
    if (!ctx) return GSRT_E_ARG;
    gsrt_status s = gsrt::sync_all(ctx);
    if (s != GSRT_OK) return s;
    if (gsrt_status cs = gsrt_comm_sync_internal(ctx); cs != GSRT_OK) return cs;
    return gsrt::check_error_word(ctx);
}

void* gsrt_stream(gsrt_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
void* gsrt_prep_stream(gsrt_ctx* ctx) { return ctx ? (void*)ctx->pstream : nullptr; }

gsrt_status gsrt_debug_streams(gsrt_ctx* ctx, void* out[8], uint32_t* n) {
    if (!ctx || !out || !n) return GSRT_E_ARG;
    const hipStream_t s[7] = {ctx->stream, ctx->prep_hi[0], ctx->prep_lo[0], ctx->prep_hi[1], ctx->prep_lo[1],
                              ctx->ustream, gsrt_comm_stream_internal(ctx)};
    for (uint32_t i = 0; i < 7; ++i) out[i] = (void*)s[i];
    out[7] = nullptr;
    *n = 7;
    return GSRT_OK;
}

void* gsrt_update_stream(gsrt_ctx* ctx) {
    if (!ctx) return nullptr;
    (void)hipSetDevice(ctx->device);
    if (!ctx->ustream) {  // (created with the context, unless GSRT_DEBUG_LAZY_STREAMS)
        if (hipStreamCreateWithFlags(&ctx->ustream, hipStreamNonBlocking) != hipSuccess) return nullptr;
        if (hipEventCreateWithFlags(&ctx->ev_copied, kSyncEventFlags) != hipSuccess) return nullptr;
    }
    return (void*)ctx->ustream;
}

gsrt_status gsrt_scene_from_params(gsrt_ctx* ctx, const gsrt_gauss_param* params, const gsrt_aabb* aabbs, uint32_t n,
                                   const float* sh, gsrt_scene** out) {
    if (!ctx || !out || (n && (!params || !aabbs)) || n > GSRT_MAX_GAUSSIANS) return GSRT_E_ARG;
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    gsrt_scene* sc = new (std::nothrow) gsrt_scene();
    if (!sc) return GSRT_E_OOM;
    sc->ctx = ctx;
    sc->n = n;
    gsrt_status s = GSRT_OK;
    if (hipMalloc(&sc->d_params, sizeof(gsrt_gauss_param) * (n ? n : 1)) != hipSuccess ||
        hipMalloc(&sc->d_aabbs, sizeof(gsrt_aabb) * (n ? n : 1)) != hipSuccess) {
        gsrt_destroy_scene(sc);
        return fail(ctx, GSRT_E_OOM, "scene allocation failed");
    }
    if (n) {
        if (hipMemcpyAsync(sc->d_params, params, sizeof(gsrt_gauss_param) * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(sc->d_aabbs, aabbs, sizeof(gsrt_aabb) * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            s = fail(ctx, GSRT_E_DEVICE, "scene upload failed");
    }
    if (s == GSRT_OK) s = upload_common(ctx, n, sh, sc);
    if (s == GSRT_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) s = fail(ctx, GSRT_E_DEVICE, "scene upload sync");
    if (s != GSRT_OK) { gsrt_destroy_scene(sc); return s; }
    *out = sc;
    return GSRT_OK;
}

gsrt_status gsrt_scene_from_model(gsrt_ctx* ctx, const float* center, const float* rot, const float* scale,
                                  const float* opacity, const float* sh, uint32_t n, gsrt_scene** out) {
    if (!ctx || !out || (n && (!center || !rot || !scale || !opacity)) || n > GSRT_MAX_GAUSSIANS) return GSRT_E_ARG;
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    gsrt_scene* sc = new (std::nothrow) gsrt_scene();
    if (!sc) return GSRT_E_OOM;
    sc->ctx = ctx;
    sc->n = n;
    float* tmp = nullptr;  // center | rot | scale | opacity staged in one block (11 floats per Gaussian)
    gsrt_status s = GSRT_OK;
    const size_t nn = n ? n : 1;
    if (hipMalloc(&sc->d_params, sizeof(gsrt_gauss_param) * nn) != hipSuccess ||
        hipMalloc(&sc->d_aabbs, sizeof(gsrt_aabb) * nn) != hipSuccess ||
        hipMalloc(&tmp, sizeof(float) * 11 * nn) != hipSuccess) {
        (void)hipFree(tmp);
        gsrt_destroy_scene(sc);
        return fail(ctx, GSRT_E_OOM, "scene allocation failed");
    }
    if (n) {
        hipStream_t st = ctx->stream;
        const auto kind = [](const void* p) { return is_device_ptr(p) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice; };
        if (hipMemcpyAsync(tmp, center, 12ull * n, kind(center), st) != hipSuccess ||
            hipMemcpyAsync(tmp + 3ull * n, rot, 16ull * n, kind(rot), st) != hipSuccess ||
            hipMemcpyAsync(tmp + 7ull * n, scale, 12ull * n, kind(scale), st) != hipSuccess ||
            hipMemcpyAsync(tmp + 10ull * n, opacity, 4ull * n, kind(opacity), st) != hipSuccess)
            s = fail(ctx, GSRT_E_DEVICE, "scene upload failed");
        if (s == GSRT_OK) {
            gsrt::launch_cov3d(st, n, tmp, tmp + 3ull * n, tmp + 7ull * n, tmp + 10ull * n, sc->d_params, sc->d_aabbs);
            if (hipGetLastError() != hipSuccess) s = fail(ctx, GSRT_E_DEVICE, "cov3d launch failed");
        }
    }
    // a device sh takes gsrt_scene_set_sh's device path: k_sh_rows, the same two float32 operations as the host fold
    const bool sh_dev = sh && n && is_device_ptr(sh);
    if (s == GSRT_OK) s = upload_common(ctx, n, sh_dev ? nullptr : sh, sc);
    if (s == GSRT_OK && sh_dev) {
        if (hipMalloc(&sc->d_sh, sizeof(float) * 48ull * n) != hipSuccess) s = fail(ctx, GSRT_E_OOM, "scene allocation failed");
        else {
            gsrt::launch_sh_rows(ctx->stream, sc->d_sh, sh, n);
            if (hipGetLastError() != hipSuccess) s = fail(ctx, GSRT_E_DEVICE, "sh rows launch failed");
        }
    }
    if (s == GSRT_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) s = fail(ctx, GSRT_E_DEVICE, "scene build sync");
    (void)hipFree(tmp);
    if (s != GSRT_OK) { gsrt_destroy_scene(sc); return s; }
    *out = sc;
    return GSRT_OK;
}

gsrt_status gsrt_scene_download(gsrt_scene* sc, gsrt_gauss_param* params, gsrt_aabb* aabbs) {
    if (!sc) return GSRT_E_ARG;
    gsrt_ctx* ctx = sc->ctx;
    if (gsrt_status s = gsrt::sync_all(ctx); s != GSRT_OK) return s;  // updates are queued on the prep stream
    if (params && sc->n)
        GSRT_HIP(ctx, hipMemcpyAsync(params, sc->d_params, sizeof(gsrt_gauss_param) * sc->n, hipMemcpyDeviceToHost, ctx->stream));
    if (aabbs && sc->n)
        GSRT_HIP(ctx, hipMemcpyAsync(aabbs, sc->d_aabbs, sizeof(gsrt_aabb) * sc->n, hipMemcpyDeviceToHost, ctx->stream));
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GSRT_OK;
}

uint32_t gsrt_scene_size(const gsrt_scene* sc) { return sc ? sc->n : 0u; }

// The table is kept as one 64-B row per Gaussian id (16 floats, channels >= C zero): the render kernel's stage DMA
// fetches a row as four 16-B pieces beside the candidate's record. A host source is padded here before the copy, a
// device source by a small kernel. No frame is in flight while the rows change (sync_all first).
gsrt_status gsrt_scene_set_features(gsrt_scene* sc, const float* feat, uint32_t channels) {
    if (!sc) return GSRT_E_ARG;
    gsrt_ctx* ctx = sc->ctx;
    if ((feat == nullptr) != (channels == 0))
        return fail(ctx, GSRT_E_ARG, "set_features: a table needs 1..16 channels, NULL with 0 channels removes it");
    if (channels > GSRT_MAX_FEATURES) return fail(ctx, GSRT_E_ARG, "set_features: more than GSRT_MAX_FEATURES channels");
    (void)hipSetDevice(ctx->device);
    if (gsrt_status s = gsrt::sync_all(ctx); s != GSRT_OK) return s;  // queued frames read the old rows
    if (!feat) {
        (void)hipFree(sc->d_feat_rows);
        sc->d_feat_rows = nullptr;
        sc->feat_channels = 0;
        return GSRT_OK;
    }
    const size_t n = sc->n;
    if (!sc->d_feat_rows) GSRT_HIP(ctx, hipMalloc(&sc->d_feat_rows, sizeof(float) * 16 * (n ? n : 1)));
    if (is_device_ptr(feat)) {
        gsrt::launch_pad_features(ctx->stream, sc->d_feat_rows, feat, sc->n, channels);
        GSRT_HIP(ctx, hipGetLastError());
    } else if (n) {
        std::vector<float> rows(16 * n, 0.0f);
        for (size_t i = 0; i < n; ++i) std::memcpy(&rows[16 * i], feat + i * channels, sizeof(float) * channels);
        GSRT_HIP(ctx, hipMemcpyAsync(sc->d_feat_rows, rows.data(), sizeof(float) * 16 * n, hipMemcpyHostToDevice, ctx->stream));
    }
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the source (and rows above) may go once the call returns
    sc->feat_channels = channels;
    return GSRT_OK;
}

uint32_t gsrt_scene_features(const gsrt_scene* sc) { return sc && sc->d_feat_rows ? sc->feat_channels : 0u; }

// The SH rows in upload_common's device layout and fold: a host source is transposed here with upload_common's own
// expression, a device source by a small kernel (k_sh_rows, the same two float32 operations). No frame is in flight while
// the rows change (sync_all first).
gsrt_status gsrt_scene_set_sh(gsrt_scene* sc, const float* sh) {
    if (!sc) return GSRT_E_ARG;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    if (gsrt_status s = gsrt::sync_all(ctx); s != GSRT_OK) return s;  // queued frames read the old rows
    if (!sh) {
        (void)hipFree(sc->d_sh);
        sc->d_sh = nullptr;
        return GSRT_OK;
    }
    const size_t n = sc->n;
    if (!sc->d_sh) GSRT_HIP(ctx, hipMalloc(&sc->d_sh, sizeof(float) * 48 * (n ? n : 1)));
    if (is_device_ptr(sh)) {
        gsrt::launch_sh_rows(ctx->stream, sc->d_sh, sh, sc->n);
        GSRT_HIP(ctx, hipGetLastError());
    } else if (n) {
        std::vector<float> t(48 * n);
        for (size_t i = 0; i < n; ++i)
            for (int c = 0; c < 3; ++c) {
                t[48 * i + 16 * c] = sh[48 * i + c] * gsrt::kShY0 + 0.5f;
                for (int k = 1; k < 16; ++k) t[48 * i + 16 * c + k] = sh[48 * i + 3 * k + c];
            }
        GSRT_HIP(ctx, hipMemcpyAsync(sc->d_sh, t.data(), sizeof(float) * 48 * n, hipMemcpyHostToDevice, ctx->stream));
    }
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the source (and t above) may go once the call returns
    return GSRT_OK;
}

void gsrt_destroy_scene(gsrt_scene* sc) {
    if (!sc) return;
    if (sc->ctx) {
        (void)hipSetDevice(sc->ctx->device);
        (void)gsrt::sync_all(sc->ctx);
    }
    // borrowed arrays (gsrt_scene_attach) are the caller's
    if (sc->attached[0]) sc->d_params = nullptr;
    if (sc->attached[1]) sc->d_aabbs = nullptr;
    // (a scene that failed before upload_common holds its arrays in d_params / d_aabbs only)
    if (sc->d_params && sc->d_params != sc->d_buf[0][0] && sc->d_params != sc->d_buf[0][1]) (void)hipFree(sc->d_params);
    if (sc->d_aabbs && sc->d_aabbs != sc->d_buf[1][0] && sc->d_aabbs != sc->d_buf[1][1]) (void)hipFree(sc->d_aabbs);
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
            (void)hipFree(sc->d_buf[a][b]);
            for (int k = 0; k < 3; ++k)
                if (sc->ev_ret[a][b][k]) (void)hipEventDestroy(sc->ev_ret[a][b][k]);
        }
    (void)hipFree(sc->d_sh);
    (void)hipFree(sc->d_feat_rows);
    (void)hipFree(sc->d_flags);
    for (uint32_t b = 0; b < kSlots; ++b) {
        (void)hipFree(sc->d_recs[b]);
        (void)hipFree(sc->d_keyed[b]);
        (void)hipFree(sc->d_inband[b]);
        (void)hipFree(sc->d_footprint[b]);
    }
    for (uint32_t b = 0; b < kSlots; ++b) {
        (void)hipFree(sc->d_nodes[b]);
        (void)hipFree(sc->d_root_box[b]);
    }
    (void)hipFree(sc->d_leaf_parent);
    (void)hipFree(sc->d_node_parent);
    (void)hipFree(sc->d_gid_slot);
    (void)hipFree(sc->d_node_range);
    for (uint32_t b = 0; b < kSlots; ++b) {
        (void)hipFree(sc->d_fit_flags[b]);
        (void)hipFree(sc->d_fit_queue[b]);
    }
    (void)hipFree(sc->d_sort);
    (void)hipFree(sc->d_leaf_gid);
    (void)hipFree(sc->d_morton);
    (void)hipFree(sc->d_tris);
    (void)hipFree(sc->d_mesh_nodes);
    delete sc;
}

gsrt_status gsrt_build_bvh(gsrt_scene* sc) {
    if (!sc) return GSRT_E_ARG;
    (void)hipSetDevice(sc->ctx->device);
    gsrt::mark_main_dirty(sc->ctx);
    gsrt_status s = gsrt::sync_all(sc->ctx);  // a rebuild may reallocate nodes an in-flight frame still reads
    return s != GSRT_OK ? s : gsrt::lbvh_build(sc);
}

// The copies of gsrt_refit_bvh / gsrt_scene_update go on the prep stream: after the prep kernels of the frames
// already queued (their projection read the old arrays), before the next frame's prep; the pipelined render
// kernels never read d_params / d_aabbs. A REF or counting render still queued on the render stream does (its
// projection and fit run there): the copies then wait for it too. The fit itself is lazy (geom_version).
// A scene array (a = 0 params, 1 AABBs) replaced from a host or device source: the copy goes into the array's other
// buffer on the update stream, which waits only for the kernels that read that buffer while it was current (recorded
// when it was retired). The buffer then becomes current: frames enqueued from now on read it, and each stream waits for
// the copy before it next reads an array (wait_updates). So frame f+1's update copy overlaps frame f's fit, projection,
// lists and render instead of queueing behind them on the prep stream (the 8-rank C5 share's chain: copies 0.41 ms of
// ~0.97 ms per frame, profiles/r06). Device sources go through gsrt::launch_copy_d2d (one-wave workgroups that loop),
// not the runtime's blit kernel, which beside a running render kernel took 2.9 ms for C5's 360 MB update.
static gsrt_status update_array(gsrt_scene* sc, int a, const void* src, size_t bytes) {
    gsrt_ctx* ctx = sc->ctx;
    if (!gsrt_update_stream(ctx)) return fail(ctx, GSRT_E_DEVICE, "update stream creation failed");
    const uint32_t c = sc->cur[a], x = c ^ 1u;
    if (!sc->d_buf[a][x]) {
        GSRT_HIP(ctx, hipMalloc(&sc->d_buf[a][x], bytes));
        for (int k = 0; k < 3; ++k) GSRT_HIP(ctx, hipEventCreateWithFlags(&sc->ev_ret[a][x][k], kSyncEventFlags));
        for (int k = 0; k < 3; ++k) GSRT_HIP(ctx, hipEventCreateWithFlags(&sc->ev_ret[a][c][k], kSyncEventFlags));
    }
    for (int k = 0; k < 3; ++k)
        if (sc->ret_rec[a][x][k]) GSRT_HIP(ctx, hipStreamWaitEvent(ctx->ustream, sc->ev_ret[a][x][k], 0));
    if (is_device_ptr(src)) {
        gsrt::launch_copy_d2d(ctx->ustream, sc->d_buf[a][x], src, bytes);
        GSRT_HIP(ctx, hipGetLastError());
    } else {
        GSRT_HIP(ctx, hipMemcpyAsync(sc->d_buf[a][x], src, bytes, hipMemcpyHostToDevice, ctx->ustream));
    }
    GSRT_HIP(ctx, hipEventRecord(ctx->ev_copied, ctx->ustream));
    ctx->copy_unseen = 0x1Fu;
    // retire the current buffer: where its readers stand on the prep streams (pipelined frames' fits and projections;
    // in slot-stream mode the second one's too) and, after a REF / counting frame, on the render stream
    const hipStream_t rs[3] = {ctx->pstream, ctx->fstream, ctx->stream};
    for (int k = 0; k < 3; ++k) {
        sc->ret_rec[a][c][k] = k < 2 || ctx->serial_reads;
        if (sc->ret_rec[a][c][k]) GSRT_HIP(ctx, hipEventRecord(sc->ev_ret[a][c][k], rs[k]));
    }
    sc->cur[a] = x;
    sc->attached[a] = nullptr;
    if (a == 0) sc->d_params = static_cast<gsrt_gauss_param*>(sc->d_buf[a][x]);
    else sc->d_aabbs = static_cast<gsrt_aabb*>(sc->d_buf[a][x]);
    ctx->scene_moved = true;
    return GSRT_OK;
}

// With slot streams, frames of slot 1 run on their own stream (fstream): the copies also wait for those
// queued there, and the next frame on each of those streams waits for the copies (launch_render).
static gsrt_status order_update(gsrt_ctx* ctx) {
    ctx->scene_moved = true;
    for (uint32_t j = 1; j < kStreamSlots; ++j) {
        if (ctx->side_frames[j]) {
            GSRT_HIP(ctx, hipEventRecord(ctx->ev_side[j], gsrt::slot_stream(ctx, j)));
            GSRT_HIP(ctx, hipStreamWaitEvent(ctx->pstream, ctx->ev_side[j], 0));
            ctx->side_frames[j] = false;
        }
        ctx->side_updates[j] = true;
    }
    if (!ctx->serial_pending) return GSRT_OK;
    GSRT_HIP(ctx, hipEventRecord(ctx->ev_serial, ctx->stream));
    GSRT_HIP(ctx, hipStreamWaitEvent(ctx->pstream, ctx->ev_serial, 0));
    ctx->serial_pending = false;
    return GSRT_OK;
}

gsrt_status gsrt_refit_bvh(gsrt_scene* sc, const gsrt_aabb* aabbs) {
    if (!sc) return GSRT_E_ARG;
    if (!sc->bvh_built) return fail(sc->ctx, GSRT_E_STATE, "refit before build");
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    if (aabbs && sc->n) {
        if (gsrt_status s = update_array(sc, 1, aabbs, sizeof(gsrt_aabb) * sc->n); s != GSRT_OK) return s;
        ++sc->aabb_version;
    }
    ctx->scene_moved = true;
    ctx->serial_reads = false;
    ++sc->geom_version;
    return GSRT_OK;
}

gsrt_status gsrt_scene_update(gsrt_scene* sc, const gsrt_gauss_param* params, const gsrt_aabb* aabbs) {
    if (!sc) return GSRT_E_ARG;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    if (!sc->n) return GSRT_OK;
    if (params)
        if (gsrt_status s = update_array(sc, 0, params, sizeof(gsrt_gauss_param) * sc->n); s != GSRT_OK) return s;
    if (aabbs) {
        if (gsrt_status s = update_array(sc, 1, aabbs, sizeof(gsrt_aabb) * sc->n); s != GSRT_OK) return s;
        ++sc->aabb_version;  // the in-band bitmaps follow the AABBs
    }
    ctx->serial_reads = false;
    return GSRT_OK;
}

// Borrowed arrays: the scene's pointer is the caller's array, so frames read it in place (no copy, no second
// buffer). The update stream's current point is recorded for the frame streams to wait on, as after a copy: a producer
// on the GPU fills the array there. The scene's own current buffer keeps its retire events; the next copy into the
// other buffer (an update, or the copy of the borrowed array itself at detach / stream_pages) retires it then.
gsrt_status gsrt_scene_attach(gsrt_scene* sc, const gsrt_gauss_param* params, const gsrt_aabb* aabbs) {
    if (!sc) return GSRT_E_ARG;
    gsrt_ctx* ctx = sc->ctx;
    (void)hipSetDevice(ctx->device);
    const void* src[2] = {params, aabbs};
    for (int a = 0; a < 2; ++a)
        if (src[a] && (!is_device_ptr(src[a]) || reinterpret_cast<uintptr_t>(src[a]) % 16u))
            return fail(ctx, GSRT_E_ARG, "attach: an array is not a 16-byte aligned device pointer");
    if (!sc->n || (!params && !aabbs)) return GSRT_OK;
    if (!gsrt_update_stream(ctx)) return fail(ctx, GSRT_E_DEVICE, "update stream creation failed");
    GSRT_HIP(ctx, hipEventRecord(ctx->ev_copied, ctx->ustream));
    ctx->copy_unseen = 0x1Fu;
    if (params) {
        sc->attached[0] = params;
        sc->d_params = const_cast<gsrt_gauss_param*>(params);
    }
    if (aabbs) {
        sc->attached[1] = aabbs;
        sc->d_aabbs = const_cast<gsrt_aabb*>(aabbs);
        ++sc->aabb_version;
    }
    ctx->scene_moved = true;
    return GSRT_OK;
}

// copy borrowed arrays into the scene's own buffers (update_array: the copy ends the borrow)
static gsrt_status take_attached(gsrt_scene* sc) {
    const size_t bytes[2] = {sizeof(gsrt_gauss_param) * sc->n, sizeof(gsrt_aabb) * sc->n};
    for (int a = 0; a < 2; ++a)
        if (sc->attached[a])
            if (gsrt_status s = update_array(sc, a, sc->attached[a], bytes[a]); s != GSRT_OK) return s;
    return GSRT_OK;
}

gsrt_status gsrt_scene_detach(gsrt_scene* sc) {
    if (!sc) return GSRT_E_ARG;
    (void)hipSetDevice(sc->ctx->device);
    if (gsrt_status s = take_attached(sc); s != GSRT_OK) return s;
    return gsrt::sync_all(sc->ctx);  // the copies and every frame that read the caller's arrays are done
}

uint32_t gsrt_scene_pages(const gsrt_scene* sc) {
    return sc ? (sc->n + GSRT_PAGE_GAUSSIANS - 1) / GSRT_PAGE_GAUSSIANS : 0u;
}

gsrt_status gsrt_scene_stream_pages(gsrt_scene* sc, const gsrt_gauss_param* params, const gsrt_aabb* aabbs,
                                    const uint32_t* pages, uint32_t npages) {
    if (!sc || (npages && !pages)) return GSRT_E_ARG;
    gsrt_ctx* ctx = sc->ctx;
    const uint32_t np = gsrt_scene_pages(sc);
    for (uint32_t i = 0; i < npages; ++i)
        if (pages[i] >= np) return fail(ctx, GSRT_E_ARG, "page id out of range");
    if (!npages || (!params && !aabbs)) return GSRT_OK;
    (void)hipSetDevice(ctx->device);
    if (gsrt_status s = take_attached(sc); s != GSRT_OK) return s;  // pages land in the scene's own arrays
    if (gsrt_status s = order_update(ctx); s != GSRT_OK) return s;
    if (gsrt_status s = gsrt::wait_updates(ctx, ctx->pstream); s != GSRT_OK) return s;  // an update's copy into them
    // runs of consecutive page ids (in the order given) become one transfer per array
    std::vector<uint32_t> ids(pages, pages + npages);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const hipMemcpyKind kp = params && is_device_ptr(params) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind ka = aabbs && is_device_ptr(aabbs) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    for (size_t i = 0; i < ids.size();) {
        size_t j = i + 1;
        while (j < ids.size() && ids[j] == ids[j - 1] + 1) ++j;
        const size_t g0 = (size_t)ids[i] * GSRT_PAGE_GAUSSIANS;
        const size_t g1 = std::min<size_t>((size_t)(ids[j - 1] + 1) * GSRT_PAGE_GAUSSIANS, sc->n);
        if (params && kp == hipMemcpyDeviceToDevice)
            gsrt::launch_copy_d2d(ctx->pstream, sc->d_params + g0, params + g0, sizeof(gsrt_gauss_param) * (g1 - g0));
        else if (params)
            GSRT_HIP(ctx, hipMemcpyAsync(sc->d_params + g0, params + g0, sizeof(gsrt_gauss_param) * (g1 - g0), kp, ctx->pstream));
        if (aabbs && ka == hipMemcpyDeviceToDevice)
            gsrt::launch_copy_d2d(ctx->pstream, sc->d_aabbs + g0, aabbs + g0, sizeof(gsrt_aabb) * (g1 - g0));
        else if (aabbs)
            GSRT_HIP(ctx, hipMemcpyAsync(sc->d_aabbs + g0, aabbs + g0, sizeof(gsrt_aabb) * (g1 - g0), ka, ctx->pstream));
        GSRT_HIP(ctx, hipGetLastError());
        i = j;
    }
    if (aabbs)
        ++sc->aabb_version;  // the in-band bitmaps follow the AABBs
    return GSRT_OK;
}

gsrt_status gsrt_host_register(gsrt_ctx* ctx, void* ptr, size_t bytes) {
    if (!ctx || !ptr || !bytes) return GSRT_E_ARG;
    (void)hipSetDevice(ctx->device);
    GSRT_HIP(ctx, hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return GSRT_OK;
}

gsrt_status gsrt_host_unregister(gsrt_ctx* ctx, void* ptr) {
    if (!ctx || !ptr) return GSRT_E_ARG;
    (void)hipSetDevice(ctx->device);
    GSRT_HIP(ctx, hipHostUnregister(ptr));
    return GSRT_OK;
}

// the BVH as the last rendered slot holds it, fitted to the current geometry (bvh_info / bvh_download)
static gsrt_status settled_bvh_slot(gsrt_scene* sc, uint32_t* slot) {
    gsrt_ctx* ctx = sc->ctx;
    gsrt_status s = gsrt::sync_all(ctx);
    if (s != GSRT_OK) return s;
    *slot = sc->last_slot;
    s = gsrt::lbvh_fit_if_stale(sc, *slot, ctx->stream, true);  // with the leaf AABBs (not a frame's footprints)
    if (s != GSRT_OK) return s;
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return GSRT_OK;
}

gsrt_status gsrt_bvh_info(gsrt_scene* sc, uint32_t* n_internal, float root_box[6], uint32_t* max_depth) {
    if (!sc) return GSRT_E_ARG;
    if (!sc->bvh_built) return fail(sc->ctx, GSRT_E_STATE, "bvh not built");
    if (n_internal) *n_internal = sc->n > 1 ? sc->n - 1 : 0;
    uint32_t slot = 0;
    gsrt_status st = settled_bvh_slot(sc, &slot);
    if (st != GSRT_OK) return st;
    if (root_box) {
        if (sc->n) GSRT_HIP(sc->ctx, hipMemcpy(root_box, sc->d_root_box[slot], sizeof(float) * 6, hipMemcpyDeviceToHost));
        else std::memset(root_box, 0, sizeof(float) * 6);
    }
    if (max_depth) {
        uint32_t depth = 0;
        if (sc->n > 1) {
            std::vector<gsrt::BvhNode> nodes(sc->n - 1);
            gsrt_ctx* ctx = sc->ctx;
            GSRT_HIP(ctx, hipMemcpy(nodes.data(), sc->d_nodes[slot], sizeof(gsrt::BvhNode) * nodes.size(), hipMemcpyDeviceToHost));
            std::vector<uint32_t> d(nodes.size(), 0);
            std::vector<uint32_t> stack{0};
            d[0] = 1;
            while (!stack.empty()) {
                uint32_t i = stack.back();
                stack.pop_back();
                for (uint32_t ref : {nodes[i].l_ref, nodes[i].r_ref}) {
                    if (ref & gsrt::kLeafBit) depth = std::max(depth, d[i] + 1);
                    else if (ref < nodes.size()) { d[ref] = d[i] + 1; stack.push_back(ref); }
                }
            }
        } else if (sc->n == 1) {
            depth = 1;
        }
        *max_depth = depth;
    }
    return GSRT_OK;
}

gsrt_status gsrt_bvh_download(gsrt_scene* sc, uint32_t* nodes, uint32_t* leaf_gid, uint32_t* morton) {
    if (!sc) return GSRT_E_ARG;
    if (!sc->bvh_built) return fail(sc->ctx, GSRT_E_STATE, "bvh not built");
    gsrt_ctx* ctx = sc->ctx;
    uint32_t slot = 0;
    gsrt_status st = settled_bvh_slot(sc, &slot);
    if (st != GSRT_OK) return st;
    if (nodes && sc->n > 1) GSRT_HIP(ctx, hipMemcpy(nodes, sc->d_nodes[slot], sizeof(gsrt::BvhNode) * (sc->n - 1), hipMemcpyDeviceToHost));
    if (leaf_gid && sc->n) GSRT_HIP(ctx, hipMemcpy(leaf_gid, sc->d_leaf_gid, 4ull * sc->n, hipMemcpyDeviceToHost));
    if (morton && sc->n) GSRT_HIP(ctx, hipMemcpy(morton, sc->d_morton, 4ull * sc->n, hipMemcpyDeviceToHost));
    return GSRT_OK;
}

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

// a blocking entry point's copy of a device result into the caller's host memory (dst nullptr: none); what: the error
struct Download {
    void* dst;
    const void* src;
    size_t bytes;
    const char* what;
};

// The tail of the blocking entry points, s the status so far: the downloads are queued only while it is GSRT_OK, the
// render stream is drained either way (then *tmp, the call's temporary device buffer, is freed), the stream's error is
// reported only if none came earlier, and the sticky error word is checked.
static gsrt_status finish_blocking(gsrt_ctx* ctx, gsrt_status s, std::initializer_list<Download> downloads,
                                   void* const* tmp = nullptr) {
    for (const Download& d : downloads)
        if (s == GSRT_OK && d.dst && hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            s = fail(ctx, GSRT_E_DEVICE, d.what);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && s == GSRT_OK)
        s = fail(ctx, GSRT_E_DEVICE, std::string("render: ") + hipGetErrorString(hipGetLastError()));
    if (tmp) (void)hipFree(*tmp);
    if (s == GSRT_OK) s = gsrt::check_error_word(ctx);
    return s;
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
    const bool in_dev = is_device_ptr(grad_splat), c_dev = is_device_ptr(grad_center), v_dev = is_device_ptr(grad_cov);
    if (accumulate && (!c_dev || !v_dev))
        return fail(ctx, GSRT_E_ARG, std::string(depth ? "gsrt_splat_depth_grad_to_model" : "gsrt_splat_grad_to_model") +
                                         ": accumulate needs device tables");
    // the host tables' device copies: one block, rows | centres | covariances
    const size_t n = sc->n, nn = n ? n : 1;
    float* tmp = nullptr;
    if (!in_dev || !c_dev || !v_dev) GSRT_HIP(ctx, hipMalloc(&tmp, sizeof(float) * 17 * nn));
    void* tmpv = tmp;
    float* const d_rows = tmp, * const d_c = tmp + 8 * nn, * const d_v = tmp + 11 * nn;
    if (!in_dev && n && hipMemcpyAsync(d_rows, grad_splat, sizeof(float) * 8 * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        s = fail(ctx, GSRT_E_DEVICE, "splat gradient upload failed");
    if (s == GSRT_OK)
        s = model_grad_async(sc, ubo, in_dev ? grad_splat : d_rows, c_dev ? grad_center : d_c, v_dev ? grad_cov : d_v,
                             accumulate, depth);
    return finish_blocking(ctx, s, {{!c_dev && n ? grad_center : nullptr, d_c, sizeof(float) * 3 * n,
                                     "centre gradient download failed"},
                                    {!v_dev && n ? grad_cov : nullptr, d_v, sizeof(float) * 6 * n,
                                     "covariance gradient download failed"}}, &tmpv);
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
    const size_t n = sc->n;
    float* tmp = nullptr;
    const bool in_dev = is_device_ptr(grad_splat) || !n;
    if (!in_dev) GSRT_HIP(ctx, hipMalloc(&tmp, sizeof(float) * 8 * n));
    void* tmpv = tmp;
    if (!in_dev && hipMemcpyAsync(tmp, grad_splat, sizeof(float) * 8 * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        s = fail(ctx, GSRT_E_DEVICE, "splat gradient upload failed");
    float* d_out = nullptr;
    if (s == GSRT_OK) s = pose_grad_enqueue(sc, ubo, in_dev ? grad_splat : tmp, depth != 0, nullptr, &d_out);
    return finish_blocking(ctx, s, {{d_out ? grad_model_view : nullptr, d_out, sizeof(float) * 16,
                                     "gsrt_pose_grad: download failed"}}, &tmpv);
}

gsrt_status gsrt_debug_pose_grad_layout(uint32_t out[2]) {
    if (!out) return GSRT_E_ARG;
    out[0] = gsrt::kPoseChunk;
    out[1] = gsrt::kPoseFinalLanes;
    return GSRT_OK;
}

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

gsrt_status gsrt_density_stats_add_async(gsrt_ctx* ctx, uint32_t n, uint32_t width, uint32_t height,
                                         const float* d_grad_splat, float* d_stats) {
    if (!ctx) return GSRT_E_ARG;
    if (!d_grad_splat || !d_stats) return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: a NULL pointer");
    if (!width || !height) return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: width and height must be non-zero");
    if (n > GSRT_MAX_GAUSSIANS) return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: n above GSRT_MAX_GAUSSIANS");
    if (reinterpret_cast<uintptr_t>(d_grad_splat) % 16u)
        return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: grad_splat must be 16-byte aligned on the device");
    (void)hipSetDevice(ctx->device);
    gsrt::launch_density_stats(ctx->stream, n, width, height, d_grad_splat, d_stats);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

gsrt_status gsrt_density_stats_add(gsrt_ctx* ctx, uint32_t n, uint32_t width, uint32_t height, const float* grad_splat,
                                   float* stats) {
    if (!ctx) return GSRT_E_ARG;
    if (!grad_splat || !stats) return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: a NULL pointer");
    if (!width || !height) return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: width and height must be non-zero");
    if (n > GSRT_MAX_GAUSSIANS) return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: n above GSRT_MAX_GAUSSIANS");
    (void)hipSetDevice(ctx->device);
    const bool dev = is_device_ptr(grad_splat);
    if (dev != is_device_ptr(stats))
        return fail(ctx, GSRT_E_ARG, "gsrt_density_stats_add: grad_splat and stats must both be host or both be device pointers");
    if (dev) return finish_blocking(ctx, gsrt_density_stats_add_async(ctx, n, width, height, grad_splat, stats), {});
    if (!n) return GSRT_OK;
    Staging tmp;
    GSRT_HIP(ctx, hipMalloc(&tmp.base, Staging::unit(sizeof(float) * 8 * n) + Staging::unit(sizeof(float) * 2 * n)));
    void* const tmpv = tmp.base;
    float* const d_rows = tmp.take<float>(8 * (size_t)n);
    float* const d_stats = tmp.take<float>(2 * (size_t)n);
    gsrt_status s = GSRT_OK;
    if (hipMemcpyAsync(d_rows, grad_splat, sizeof(float) * 8 * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(d_stats, stats, sizeof(float) * 2 * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        s = fail(ctx, GSRT_E_DEVICE, "density statistic upload failed");
    if (s == GSRT_OK) s = gsrt_density_stats_add_async(ctx, n, width, height, d_rows, d_stats);
    return finish_blocking(ctx, s, {{stats, d_stats, sizeof(float) * 2 * n, "density statistic download failed"}}, &tmpv);
}

gsrt_status gsrt_densify_count(gsrt_ctx* ctx, uint32_t n, const float* scale, const float* opacity, const float* stats,
                               const gsrt_densify_params* params, uint32_t* n_out) {
    if (!ctx) return GSRT_E_ARG;
    if (!n_out || (n && (!scale || !opacity || !stats))) return fail(ctx, GSRT_E_ARG, "gsrt_densify_count: a NULL pointer");
    if (n > GSRT_MAX_GAUSSIANS) return fail(ctx, GSRT_E_ARG, "gsrt_densify_count: n above GSRT_MAX_GAUSSIANS");
    gsrt_status s = check_densify_params(ctx, "gsrt_densify_count", params);
    if (s != GSRT_OK) return s;
    *n_out = 0;
    if (!n) return GSRT_OK;
    (void)hipSetDevice(ctx->device);
    if ((s = densify_workspace(ctx, n)) != GSRT_OK) return s;
    const float* src[3] = {scale, opacity, stats};
    const size_t floats[3] = {3 * (size_t)n, (size_t)n, 2 * (size_t)n};
    Staging tmp;
    size_t bytes = 0;
    for (int a = 0; a < 3; ++a)
        if (!is_device_ptr(src[a])) bytes += Staging::unit(sizeof(float) * floats[a]);
    if (bytes) GSRT_HIP(ctx, hipMalloc(&tmp.base, bytes));
    void* const tmpv = tmp.base;
    for (int a = 0; a < 3 && s == GSRT_OK; ++a)
        if (!is_device_ptr(src[a])) {
            float* d = tmp.take<float>(floats[a]);
            if (hipMemcpyAsync(d, src[a], sizeof(float) * floats[a], hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
                s = fail(ctx, GSRT_E_DEVICE, "gsrt_densify_count: upload failed");
            src[a] = d;
        }
    uint32_t* const d_n = ctx->d_densify_ws + gsrt::densify_blocks(n);
    if (s == GSRT_OK) {
        gsrt::launch_densify_count(ctx->stream, n, *params, src[0], src[1], src[2], ctx->d_densify_ws, d_n);
        if (hipGetLastError() != hipSuccess) s = fail(ctx, GSRT_E_DEVICE, "gsrt_densify_count: launch failed");
    }
    return finish_blocking(ctx, s, {{n_out, d_n, sizeof(uint32_t), "gsrt_densify_count: download failed"}}, &tmpv);
}

// the arrays of a model in a fixed order with their floats per Gaussian (SH and features only when present)
struct ModelField {
    float* gsrt_model_arrays::*member;
    uint32_t floats;
};
static uint32_t model_fields(const gsrt_model_arrays& m, ModelField out[6]) {
    uint32_t k = 0;
    out[k++] = {&gsrt_model_arrays::center, 3};
    out[k++] = {&gsrt_model_arrays::rot_rxyz, 4};
    out[k++] = {&gsrt_model_arrays::scale, 3};
    out[k++] = {&gsrt_model_arrays::opacity, 1};
    if (m.sh) out[k++] = {&gsrt_model_arrays::sh, 48};
    if (m.features) out[k++] = {&gsrt_model_arrays::features, m.feature_channels};
    return k;
}

// what both forms of gsrt_densify refuse before anything is queued
static gsrt_status check_densify_args(gsrt_ctx* ctx, const gsrt_model_arrays* in, uint32_t n, const float* stats,
                                      const float* noise, const gsrt_densify_params* params, const gsrt_model_arrays* out,
                                      const int32_t* origin, uint32_t cap, const uint32_t* n_out) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = "gsrt_densify: ";
    if (!in || !out || !n_out) return fail(ctx, GSRT_E_ARG, name + "in, out or n_out is NULL");
    if (gsrt_status s = check_densify_params(ctx, "gsrt_densify", params); s != GSRT_OK) return s;
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
static gsrt_status densify_enqueue(gsrt_ctx* ctx, const gsrt_model_arrays& in, uint32_t n, const float* d_stats,
                                   const float* d_noise, const gsrt_densify_params& P, const gsrt_model_arrays& out,
                                   int32_t* d_origin, uint32_t cap, uint32_t* d_n_out) {
    if ((reinterpret_cast<uintptr_t>(in.sh) | reinterpret_cast<uintptr_t>(out.sh)) % 16u)
        return fail(ctx, GSRT_E_ARG, "gsrt_densify: sh must be 16-byte aligned on the device");
    if (gsrt_status s = densify_workspace(ctx, n); s != GSRT_OK) return s;
    gsrt::launch_densify_count(ctx->stream, n, P, in.scale, in.opacity, d_stats, ctx->d_densify_ws, d_n_out);
    gsrt::launch_densify_write(ctx->stream, n, P, in, d_stats, d_noise, out, d_origin, cap, ctx->d_densify_ws, d_n_out);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

gsrt_status gsrt_densify_async(gsrt_ctx* ctx, const gsrt_model_arrays* in, uint32_t n, const float* d_stats,
                               const float* d_noise, const gsrt_densify_params* params, const gsrt_model_arrays* out,
                               int32_t* d_origin, uint32_t cap, uint32_t* d_n_out) {
    gsrt_status s = check_densify_args(ctx, in, n, d_stats, d_noise, params, out, d_origin, cap, d_n_out);
    if (s != GSRT_OK) return s;
    (void)hipSetDevice(ctx->device);
    return densify_enqueue(ctx, *in, n, d_stats, d_noise, *params, *out, d_origin, cap, d_n_out);
}

gsrt_status gsrt_densify(gsrt_ctx* ctx, const gsrt_model_arrays* in, uint32_t n, const float* stats, const float* noise,
                         const gsrt_densify_params* params, const gsrt_model_arrays* out, int32_t* origin, uint32_t cap,
                         uint32_t* n_out) {
    gsrt_status s = check_densify_args(ctx, in, n, stats, noise, params, out, origin, cap, n_out);
    if (s != GSRT_OK) return s;
    *n_out = 0;
    if (!n) return GSRT_OK;
    (void)hipSetDevice(ctx->device);
    ModelField f[6];
    const uint32_t nf = model_fields(*in, f);
    // all on the host or all on the device (absent arrays take no side)
    uint32_t on_dev = 0, given = 0;
    const auto side = [&](const void* p) {
        if (!p) return;
        ++given;
        if (is_device_ptr(p)) ++on_dev;
    };
    for (uint32_t a = 0; a < nf; ++a) {
        side(in->*f[a].member);
        side(out->*f[a].member);
    }
    side(stats);
    side(noise);
    side(origin);
    if (on_dev && on_dev != given)
        return fail(ctx, GSRT_E_ARG, "gsrt_densify: the arrays must all be host pointers or all be device pointers");
    if ((s = densify_workspace(ctx, n)) != GSRT_OK) return s;
    uint32_t* const d_n = ctx->d_densify_ws + gsrt::densify_blocks(n);
    const auto refuse = [&](uint32_t rows) {
        return fail(ctx, GSRT_E_ARG, "gsrt_densify: " + std::to_string(rows) + " output rows needed, cap is " +
                                         std::to_string(cap) + " (at most GSRT_MAX_GAUSSIANS rows)");
    };
    if (on_dev) {
        s = densify_enqueue(ctx, *in, n, stats, noise, *params, *out, origin, cap, d_n);
        s = finish_blocking(ctx, s, {{n_out, d_n, sizeof(uint32_t), "gsrt_densify: count download failed"}});
        if (s == GSRT_OK && (*n_out > cap || *n_out > GSRT_MAX_GAUSSIANS)) return refuse(*n_out);
        return s;
    }
    // host arrays: one device block, inputs | stats | noise | outputs | origin
    size_t bytes = Staging::unit(sizeof(float) * 2 * n) + Staging::unit(sizeof(float) * 6 * n) +
                   Staging::unit(sizeof(int32_t) * (size_t)cap);
    for (uint32_t a = 0; a < nf; ++a)
        bytes += Staging::unit(sizeof(float) * f[a].floats * n) + Staging::unit(sizeof(float) * f[a].floats * (size_t)cap);
    Staging tmp;
    GSRT_HIP(ctx, hipMalloc(&tmp.base, bytes));
    void* const tmpv = tmp.base;
    gsrt_model_arrays d_in = *in, d_out = *out;
    const auto upload = [&](const float* src, size_t floats) {
        float* d = tmp.take<float>(floats);
        if (s == GSRT_OK && hipMemcpyAsync(d, src, sizeof(float) * floats, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            s = fail(ctx, GSRT_E_DEVICE, "gsrt_densify: upload failed");
        return d;
    };
    for (uint32_t a = 0; a < nf; ++a) d_in.*f[a].member = upload(in->*f[a].member, (size_t)f[a].floats * n);
    const float* const d_stats = upload(stats, 2 * (size_t)n);
    const float* const d_noise = upload(noise, 6 * (size_t)n);
    for (uint32_t a = 0; a < nf; ++a) d_out.*f[a].member = tmp.take<float>((size_t)f[a].floats * cap);
    int32_t* const d_origin = tmp.take<int32_t>(cap);
    if (s == GSRT_OK) s = densify_enqueue(ctx, d_in, n, d_stats, d_noise, *params, d_out, d_origin, cap, d_n);
    if (s == GSRT_OK && (hipMemcpyAsync(n_out, d_n, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                         hipStreamSynchronize(ctx->stream) != hipSuccess))
        s = fail(ctx, GSRT_E_DEVICE, "gsrt_densify: count download failed");
    if (s == GSRT_OK && (*n_out > cap || *n_out > GSRT_MAX_GAUSSIANS)) s = refuse(*n_out);
    const size_t rows = s == GSRT_OK ? *n_out : 0;
    for (uint32_t a = 0; a < nf && rows; ++a)
        if (s == GSRT_OK && hipMemcpyAsync(out->*f[a].member, d_out.*f[a].member, sizeof(float) * f[a].floats * rows,
                                           hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            s = fail(ctx, GSRT_E_DEVICE, "gsrt_densify: download failed");
    return finish_blocking(ctx, s, {{rows ? origin : nullptr, d_origin, sizeof(int32_t) * rows,
                                     "gsrt_densify: origin download failed"}}, &tmpv);
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
    const bool dev = is_device_ptr(rgba);
    if (dev != is_device_ptr(target) || (grad_image && dev != is_device_ptr(grad_image)))
        return fail(ctx, GSRT_E_ARG, "gsrt_image_loss: rgba, target and grad_image must all be host pointers or all be device pointers");
    if (is_device_ptr(out)) return fail(ctx, GSRT_E_ARG, "gsrt_image_loss: out is a host pointer");
    const size_t px = (size_t)width * height;
    float* d_out = nullptr;
    if (dev) {
        s = image_loss_enqueue(ctx, width, height, rgba, target, target_channels, lambda, nullptr, grad_image, &d_out);
        return finish_blocking(ctx, s, {{out, d_out, sizeof(float) * 4, "gsrt_image_loss: scalar download failed"}});
    }
    // host images: one device block, rgba | target | gradient
    Staging tmp;
    GSRT_HIP(ctx, hipMalloc(&tmp.base, Staging::unit(sizeof(float) * 4 * px) + Staging::unit(sizeof(float) * target_channels * px) +
                                           (grad_image ? Staging::unit(sizeof(float) * 4 * px) : 0)));
    void* const tmpv = tmp.base;
    float* const d_rgba = tmp.take<float>(4 * px);
    float* const d_target = tmp.take<float>(target_channels * px);
    float* const d_grad = grad_image ? tmp.take<float>(4 * px) : nullptr;
    if (hipMemcpyAsync(d_rgba, rgba, sizeof(float) * 4 * px, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(d_target, target, sizeof(float) * target_channels * px, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        s = fail(ctx, GSRT_E_DEVICE, "gsrt_image_loss: upload failed");
    if (s == GSRT_OK)
        s = image_loss_enqueue(ctx, width, height, d_rgba, d_target, target_channels, lambda, nullptr, d_grad, &d_out);
    return finish_blocking(ctx, s, {{out, d_out, sizeof(float) * 4, "gsrt_image_loss: scalar download failed"},
                                    {grad_image, d_grad, sizeof(float) * 4 * px, "gsrt_image_loss: gradient download failed"}},
                           &tmpv);
}

// ---- frame loss (gsrt_image_loss.hip): gsrt_image_loss over a background, under a mask, with a depth term ------------
// what both forms of gsrt_frame_loss refuse before anything is queued or written
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
    if (!(P->lambda >= 0.0f && P->lambda <= 1.0f)) return fail(ctx, GSRT_E_ARG, name + "params.lambda must be in [0, 1]");
    if (P->flags & ~GSRT_LOSS_BACKGROUND) return fail(ctx, GSRT_E_ARG, name + "an unknown flag in params.flags");
    if (P->reserved) return fail(ctx, GSRT_E_ARG, name + "params.reserved must be zero");
    if (P->flags & GSRT_LOSS_BACKGROUND)
        for (float b : P->background)
            if (!std::isfinite(b)) return fail(ctx, GSRT_E_ARG, name + "params.background must be finite");
    if (!(P->depth_weight >= 0.0f)) return fail(ctx, GSRT_E_ARG, name + "params.depth_weight is negative or NaN");
    if (!(P->alpha_min > 0.0f && P->alpha_min <= 1.0f)) return fail(ctx, GSRT_E_ARG, name + "params.alpha_min must be in (0, 1]");
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
    const bool dev = is_device_ptr(rgba);
    for (const float* p : {target, mask, depth, target_depth, (const float*)grad_image, (const float*)grad_depth})
        if (p && dev != is_device_ptr(p))
            return fail(ctx, GSRT_E_ARG, "gsrt_frame_loss: the images and gradients must all be host pointers or all be device pointers");
    if (is_device_ptr(out)) return fail(ctx, GSRT_E_ARG, "gsrt_frame_loss: out is a host pointer");
    const size_t px = (size_t)width * height, f = sizeof(float);
    const size_t scalars = f * GSRT_FRAME_LOSS_SCALARS;
    float* d_out = nullptr;
    if (dev) {
        s = frame_loss_enqueue(ctx, width, height, rgba, target, target_channels, mask, depth, target_depth, *params,
                               nullptr, grad_image, grad_depth, &d_out);
        return finish_blocking(ctx, s, {{out, d_out, scalars, "gsrt_frame_loss: scalar download failed"}});
    }
    // host images: one device block, rgba | target | mask | depth | target depth | the two gradients
    Staging tmp;
    GSRT_HIP(ctx, hipMalloc(&tmp.base, Staging::unit(f * 4 * px) + Staging::unit(f * target_channels * px) +
                                           (mask ? Staging::unit(f * px) : 0) + (depth ? 2 * Staging::unit(f * px) : 0) +
                                           (grad_image ? Staging::unit(f * 4 * px) : 0) +
                                           (grad_depth ? Staging::unit(f * px) : 0)));
    void* const tmpv = tmp.base;
    const auto upload = [&](const float* src, size_t floats) -> float* {
        if (!src) return nullptr;
        float* const d = tmp.take<float>(floats);
        if (s == GSRT_OK && hipMemcpyAsync(d, src, f * floats, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            s = fail(ctx, GSRT_E_DEVICE, "gsrt_frame_loss: upload failed");
        return d;
    };
    const float* const d_rgba = upload(rgba, 4 * px);
    const float* const d_target = upload(target, target_channels * px);
    const float* const d_mask = upload(mask, px);
    const float* const d_depth = upload(depth, px);
    const float* const d_target_depth = upload(target_depth, px);
    float* const d_grad = grad_image ? tmp.take<float>(4 * px) : nullptr;
    float* const d_grad_depth = grad_depth ? tmp.take<float>(px) : nullptr;
    if (s == GSRT_OK)
        s = frame_loss_enqueue(ctx, width, height, d_rgba, d_target, target_channels, d_mask, d_depth, d_target_depth,
                               *params, nullptr, d_grad, d_grad_depth, &d_out);
    return finish_blocking(ctx, s, {{out, d_out, scalars, "gsrt_frame_loss: scalar download failed"},
                                    {grad_image, d_grad, f * 4 * px, "gsrt_frame_loss: gradient download failed"},
                                    {grad_depth, d_grad_depth, f * px, "gsrt_frame_loss: depth gradient download failed"}},
                           &tmpv);
}

// ---- the optimiser step (gsrt_model_step.hip) -----------------------------------------------------------------------
// On the render stream, behind the gradient calls that filled the tables. The calls work on model arrays, not on a scene.
static const char* check_adam(const gsrt_adam_params* A) {
    if (!A) return "adam is NULL";
    if (A->step == 0) return "adam.step must be >= 1";
    if (!(A->beta1 >= 0.0f && A->beta1 < 1.0f) || !(A->beta2 >= 0.0f && A->beta2 < 1.0f)) return "adam.beta1 and beta2 must be in [0, 1)";
    if (!(A->eps > 0.0f)) return "adam.eps must be > 0";
    for (float lr : {A->lr_center, A->lr_rot, A->lr_scale, A->lr_opacity, A->lr_sh_dc, A->lr_sh_rest, A->lr_features})
        if (!(lr >= 0.0f)) return "a learning rate is negative or NaN";
    if (A->reserved[0] | A->reserved[1] | A->reserved[2] | A->reserved[3]) return "adam.reserved must be zero";
    if (A->flags & ~GSRT_ADAM_SPARSE) return "an unknown flag in adam.flags";
    return nullptr;
}

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

// One array of a model call: where its pointer stands (in the call's own copies of the structs), its size, and whether
// the call reads and writes it. The list drives the NULL, overlap and side checks and the host form's staging.
struct StepArray {
    float** slot;
    size_t bytes;
    bool in, out;
};

static void model_set_arrays(std::vector<StepArray>& list, gsrt_model_arrays& a, size_t n, bool in, bool out) {
    ModelField f[6];
    const uint32_t nf = model_fields(a, f);
    for (uint32_t i = 0; i < nf; ++i) list.push_back({&(a.*f[i].member), sizeof(float) * f[i].floats * n, in, out});
}

// structs that must agree on sh, features and the channel count (a nullptr entry is an absent optional struct)
static const char* check_model_sets(std::initializer_list<const gsrt_model_arrays*> sets, const gsrt_model_arrays& first) {
    for (const gsrt_model_arrays* a : sets) {
        if (!a) continue;
        if (a->feature_channels > GSRT_MAX_FEATURES || (a->features == nullptr) != (a->feature_channels == 0))
            return "features need 1..GSRT_MAX_FEATURES channels, NULL exactly with 0 channels";
        if ((a->sh == nullptr) != (first.sh == nullptr) || a->feature_channels != first.feature_channels)
            return "the structs must agree on sh, features and feature_channels";
    }
    return nullptr;
}

// NULL arrays (n > 0), overlaps of a written array with any other (same: pairs of slots that may be one array), and the
// side: 0 host, 1 device, -1 refused
static int check_step_arrays(gsrt_ctx* ctx, const std::string& name, const std::vector<StepArray>& list, size_t n,
                             std::initializer_list<std::pair<float**, float**>> same) {
    if (!n) return 1;
    for (const StepArray& a : list)
        if (!*a.slot) return fail(ctx, GSRT_E_ARG, name + "a NULL array"), -1;
    for (size_t i = 0; i < list.size(); ++i)
        for (size_t j = i + 1; j < list.size(); ++j) {
            if (!list[i].out && !list[j].out) continue;
            const uintptr_t a = reinterpret_cast<uintptr_t>(*list[i].slot), b = reinterpret_cast<uintptr_t>(*list[j].slot);
            if (!(a < b + list[j].bytes && b < a + list[i].bytes)) continue;
            bool allowed = false;
            for (const auto& p : same)
                if (a == b && ((p.first == list[i].slot && p.second == list[j].slot) ||
                               (p.first == list[j].slot && p.second == list[i].slot)))
                    allowed = true;
            if (!allowed) return fail(ctx, GSRT_E_ARG, name + "an output array overlaps another array of the call"), -1;
        }
    size_t on_dev = 0;
    for (const StepArray& a : list)
        if (is_device_ptr(*a.slot)) ++on_dev;
    if (on_dev && on_dev != list.size())
        return fail(ctx, GSRT_E_ARG, name + "the arrays must all be host pointers or all be device pointers"), -1;
    return on_dev ? 1 : 0;
}

// The host form: every array gets a region of one device block (slots that hold the same host array share one), inputs
// are uploaded, `run` enqueues the kernels on the slots' device pointers, outputs are downloaded, the stream is drained.
static gsrt_status run_staged(gsrt_ctx* ctx, const std::string& name, std::vector<StepArray>& list,
                              const std::function<gsrt_status()>& run) {
    size_t bytes = 0;
    for (const StepArray& a : list) bytes += Staging::unit(a.bytes);
    Staging tmp;
    GSRT_HIP(ctx, hipMalloc(&tmp.base, bytes ? bytes : 16));
    void* const tmpv = tmp.base;
    gsrt_status s = GSRT_OK;
    std::vector<float*> host(list.size()), dev(list.size());
    for (size_t i = 0; i < list.size(); ++i) {
        host[i] = *list[i].slot;
        dev[i] = nullptr;
        for (size_t j = 0; j < i; ++j)
            if (host[j] == host[i]) dev[i] = dev[j];
        if (!dev[i]) {
            dev[i] = tmp.take<float>(list[i].bytes / sizeof(float));
            if (list[i].in && s == GSRT_OK && list[i].bytes &&
                hipMemcpyAsync(dev[i], host[i], list[i].bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
                s = fail(ctx, GSRT_E_DEVICE, name + "upload failed");
        }
        *list[i].slot = dev[i];
    }
    if (s == GSRT_OK) s = run();
    for (size_t i = 0; i < list.size(); ++i)
        if (list[i].out && s == GSRT_OK && list[i].bytes &&
            hipMemcpyAsync(host[i], dev[i], list[i].bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            s = fail(ctx, GSRT_E_DEVICE, name + "download failed");
    return finish_blocking(ctx, s, {}, &tmpv);
}

// gsrt_model_step (adam != nullptr) and gsrt_model_activate (everything about m, v, grads absent) in one body
static gsrt_status model_step_any(gsrt_ctx* ctx, const char* fn, bool blocking, uint32_t n, const gsrt_model_arrays* raw,
                                  const gsrt_model_arrays* m, const gsrt_model_arrays* v, const gsrt_model_grads* grads,
                                  const gsrt_adam_params* adam, bool step, const gsrt_model_arrays* act,
                                  gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out, float* grad_raw) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = std::string(fn) + ": ";
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
    float* p_out = reinterpret_cast<float*>(params_out);
    float* b_out = reinterpret_cast<float*>(aabbs_out);
    std::vector<StepArray> list;
    model_set_arrays(list, r, n, true, step);
    if (step) {
        model_set_arrays(list, mm, n, true, true);
        model_set_arrays(list, vv, n, true, true);
        const auto in = [&](const float*& p, size_t floats) {
            list.push_back({const_cast<float**>(&p), sizeof(float) * floats * n, true, false});
        };
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
    if (p_out) list.push_back({&p_out, sizeof(gsrt_gauss_param) * (size_t)n, false, true});
    if (b_out) list.push_back({&b_out, sizeof(gsrt_aabb) * (size_t)n, false, true});
    if (step && grad_raw) list.push_back({&grad_raw, sizeof(float) * 11 * (size_t)n, false, true});
    if (n && (!r.center || !r.rot_rxyz || !r.scale || !r.opacity ||
              (step && (!mm.center || !mm.rot_rxyz || !mm.scale || !mm.opacity || !vv.center || !vv.rot_rxyz || !vv.scale ||
                        !vv.opacity || !gg.center || !gg.cov || !gg.splat))))
        return fail(ctx, GSRT_E_ARG, name + "a NULL array");
    const int side = check_step_arrays(ctx, name, list, n, {{&aa.sh, &r.sh}, {&aa.features, &r.features}});
    if (side < 0) return GSRT_E_ARG;
    if (!blocking && side == 0 && n) return fail(ctx, GSRT_E_ARG, name + "the async form takes device pointers only");
    gsrt::AdamScalars K{};
    if (step) adam_scalars(*adam, K);
    const auto run = [&]() -> gsrt_status {
        gsrt::launch_model_step(ctx->stream, n, step ? &K : nullptr, r, &mm, &vv, &gg, aa,
                                reinterpret_cast<gsrt_gauss_param*>(p_out), reinterpret_cast<gsrt_aabb*>(b_out), grad_raw);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GSRT_E_DEVICE, name + "launch failed");
        return GSRT_OK;
    };
    if (!n) return GSRT_OK;
    if (side == 1) {
        const gsrt_status s = run();
        return blocking ? finish_blocking(ctx, s, {}) : s;
    }
    return run_staged(ctx, name, list, run);
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
    std::vector<StepArray> list;
    model_set_arrays(list, a, n, true, false);
    model_set_arrays(list, r, n, false, true);
    const int side = check_step_arrays(ctx, name, list, n, {{&a.sh, &r.sh}, {&a.features, &r.features}});
    if (side < 0) return GSRT_E_ARG;
    if (!blocking && side == 0 && n) return fail(ctx, GSRT_E_ARG, name + "the async form takes device pointers only");
    const auto run = [&]() -> gsrt_status {
        gsrt::launch_model_deactivate(ctx->stream, n, a, r);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GSRT_E_DEVICE, name + "launch failed");
        return GSRT_OK;
    };
    if (!n) return GSRT_OK;
    if (side == 1) {
        const gsrt_status s = run();
        return blocking ? finish_blocking(ctx, s, {}) : s;
    }
    return run_staged(ctx, name, list, run);
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
    float* org = reinterpret_cast<float*>(const_cast<int32_t*>(origin));
    if (n_out && (!org || !a.center || !a.rot_rxyz || !a.scale || !a.opacity || !r.center || !r.rot_rxyz || !r.scale ||
                  !r.opacity))
        return fail(ctx, GSRT_E_ARG, name + "a NULL array");
    if (!n_out) return GSRT_OK;
    size_t n_in = 1;
    if (!is_device_ptr(origin)) {
        int64_t rows = 0;
        for (uint32_t i = 0; i < n_out; ++i) rows = std::max<int64_t>(rows, (int64_t)origin[i] + 1);
        n_in = (size_t)rows;
    }
    std::vector<StepArray> list;
    model_set_arrays(list, a, n_in, true, false);
    model_set_arrays(list, r, n_out, false, true);
    list.push_back({&org, sizeof(int32_t) * (size_t)n_out, true, false});
    const int side = check_step_arrays(ctx, name, list, n_out, {});
    if (side < 0) return GSRT_E_ARG;
    if (!blocking && side == 0) return fail(ctx, GSRT_E_ARG, name + "the async form takes device pointers only");
    const auto run = [&]() -> gsrt_status {
        gsrt::launch_model_remap(ctx->stream, n_out, reinterpret_cast<const int32_t*>(org), a, r);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GSRT_E_DEVICE, name + "launch failed");
        return GSRT_OK;
    };
    if (side == 1) {
        const gsrt_status s = run();
        return blocking ? finish_blocking(ctx, s, {}) : s;
    }
    return run_staged(ctx, name, list, run);
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
    if (is_device_ptr(out)) return finish_blocking(ctx, gsrt_normal_noise_async(ctx, count, seed, stream_id, out), {});
    (void)hipSetDevice(ctx->device);
    float* d = nullptr;
    if (hipMalloc(&d, sizeof(float) * count) != hipSuccess) return fail(ctx, GSRT_E_OOM, "gsrt_normal_noise: device allocation failed");
    void* const tmpv = d;
    gsrt::launch_normal_noise(ctx->stream, count, seed, stream_id, d);
    gsrt_status s = hipGetLastError() == hipSuccess ? GSRT_OK : fail(ctx, GSRT_E_DEVICE, "gsrt_normal_noise: launch failed");
    return finish_blocking(ctx, s, {{out, d, sizeof(float) * count, "gsrt_normal_noise: download failed"}}, &tmpv);
}

static gsrt_status opacity_reset_any(gsrt_ctx* ctx, bool blocking, uint32_t n, float* logit, float* m, float* v,
                                     float max_opacity) {
    if (!ctx) return GSRT_E_ARG;
    const std::string name = "gsrt_model_opacity_reset: ";
    if (!(max_opacity > 0.0f && max_opacity < 1.0f)) return fail(ctx, GSRT_E_ARG, name + "max_opacity must be in (0, 1)");
    if (n > GSRT_MAX_GAUSSIANS) return fail(ctx, GSRT_E_ARG, name + "n above GSRT_MAX_GAUSSIANS");
    (void)hipSetDevice(ctx->device);
    std::vector<StepArray> list = {{&logit, sizeof(float) * (size_t)n, true, true},
                                   {&m, sizeof(float) * (size_t)n, false, true},
                                   {&v, sizeof(float) * (size_t)n, false, true}};
    const int side = check_step_arrays(ctx, name, list, n, {});
    if (side < 0) return GSRT_E_ARG;
    if (!blocking && side == 0 && n) return fail(ctx, GSRT_E_ARG, name + "the async form takes device pointers only");
    const float limit = (float)std::log((double)max_opacity / (1.0 - (double)max_opacity));
    const auto run = [&]() -> gsrt_status {
        gsrt::launch_opacity_reset(ctx->stream, n, limit, logit, m, v);
        if (hipGetLastError() != hipSuccess) return fail(ctx, GSRT_E_DEVICE, name + "launch failed");
        return GSRT_OK;
    };
    if (!n) return GSRT_OK;
    if (side == 1) {
        const gsrt_status s = run();
        return blocking ? finish_blocking(ctx, s, {}) : s;
    }
    return run_staged(ctx, name, list, run);
}
gsrt_status gsrt_model_opacity_reset(gsrt_ctx* ctx, uint32_t n, float* logit_opacity, float* m_opacity, float* v_opacity,
                                     float max_opacity) {
    return opacity_reset_any(ctx, true, n, logit_opacity, m_opacity, v_opacity, max_opacity);
}
gsrt_status gsrt_model_opacity_reset_async(gsrt_ctx* ctx, uint32_t n, float* d_logit_opacity, float* d_m_opacity,
                                           float* d_v_opacity, float max_opacity) {
    return opacity_reset_any(ctx, false, n, d_logit_opacity, d_m_opacity, d_v_opacity, max_opacity);
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

gsrt_status gsrt_timing(gsrt_ctx* ctx, uint32_t frames) {
    if (!ctx) return GSRT_E_ARG;
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    while (ctx->events.size() < (size_t)gsrt::kTimingEvents * frames) {
        hipEvent_t e;
        GSRT_HIP(ctx, hipEventCreateWithFlags(&e, kTimingEventFlags));
        ctx->events.push_back(e);
    }
    if (ctx->timing_ex.size() < frames) ctx->timing_ex.resize(frames, 0);
    ctx->timing_cap = frames;
    ctx->timing_n = 0;
    ctx->timing_kernel_only = ctx->timing_kernel_only_next;
    ctx->timing_stride = ctx->timing_stride_next;
    ctx->timing_frame = 0;
    return GSRT_OK;
}

gsrt_status gsrt_timing_read(gsrt_ctx* ctx, float* kernel_ms, float* frame_ms, uint32_t cap, uint32_t* nframes) {
    if (!ctx) return GSRT_E_ARG;
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t n = ctx->timing_n < cap ? ctx->timing_n : cap;
    for (uint32_t i = 0; i < n; ++i) {
        float k = 0.f, f = 0.f;
        const size_t e = (size_t)gsrt::kTimingEvents * i;
        GSRT_HIP(ctx, hipEventElapsedTime(&k, ctx->events[e + 1], ctx->events[e + 2]));
        if (!ctx->timing_kernel_only) GSRT_HIP(ctx, hipEventElapsedTime(&f, ctx->events[e + 0], ctx->events[e + 3]));
        if (kernel_ms) kernel_ms[i] = k;
        if (frame_ms) frame_ms[i] = f;
    }
    if (nframes) *nframes = n;
    return GSRT_OK;
}

gsrt_status gsrt_timing_kernel_only(gsrt_ctx* ctx, int on) {
    if (!ctx) return GSRT_E_ARG;
    ctx->timing_kernel_only_next = on != 0;
    return GSRT_OK;
}

gsrt_status gsrt_timing_stride(gsrt_ctx* ctx, uint32_t stride) {
    if (!ctx || stride == 0) return GSRT_E_ARG;
    ctx->timing_stride_next = stride;
    return GSRT_OK;
}

// diagnostic: raw counter block of the last render (16 words; [9..11] are cycle sums in GSRT_DIAG builds)
gsrt_status gsrt_debug_counters(gsrt_ctx* ctx, uint64_t out[16]) {
    if (!ctx || !out) return GSRT_E_ARG;
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    GSRT_HIP(ctx, hipMemcpy(out, ctx->d_counters, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost));
    return GSRT_OK;
}

// diagnostic: words 16..31 of the counter block (GSRT_DIAG builds: shading-loop wave-candidate counts)
gsrt_status gsrt_debug_counters_hi(gsrt_ctx* ctx, uint64_t out[16]) {
    if (!ctx || !out) return GSRT_E_ARG;
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    GSRT_HIP(ctx, hipMemcpy(out, ctx->d_counters + 16, sizeof(unsigned long long) * 16, hipMemcpyDeviceToHost));
    return GSRT_OK;
}

gsrt_status gsrt_exp_lut(float out[512]) {
    if (!out) return GSRT_E_ARG;
    gsrt::exp_lut(out);
    return GSRT_OK;
}

gsrt_status gsrt_debug_exp_lut(gsrt_ctx* ctx, float out[512]) {
    if (!ctx || !out) return GSRT_E_ARG;
    GSRT_HIP(ctx, hipMemcpy(out, ctx->d_lut, sizeof(float) * 512, hipMemcpyDeviceToHost));
    return GSRT_OK;
}

const float* gsrt_framebuffer(gsrt_ctx* ctx) { return ctx && !ctx->fb_dump8 ? gsrt::framebuffer_of(ctx) : nullptr; }
int gsrt_slot_streams(const gsrt_ctx* ctx) { return ctx && ctx->last_slot_streams ? 1 : 0; }

gsrt_status gsrt_vs_stats(gsrt_ctx* ctx, uint64_t out[8]) {
    if (!ctx || !out) return GSRT_E_ARG;
    if (!ctx->last_stats || !ctx->last_ref) return fail(ctx, GSRT_E_STATE, "last render was not a REF render with GSRT_FLAG_STATS");
    unsigned long long c[32];
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    GSRT_HIP(ctx, hipMemcpy(c, ctx->d_counters, sizeof c, hipMemcpyDeviceToHost));
    const uint64_t v[8] = {c[29], c[26], c[27], c[25], c[24], c[28], 0, 0};
    std::memcpy(out, v, sizeof v);
    return GSRT_OK;
}

gsrt_status gsrt_dump_vs_stats(gsrt_ctx* ctx, const char* path) {
    uint64_t v[8];
    if (!path) return GSRT_E_ARG;
    if (gsrt_status s = gsrt_vs_stats(ctx, v); s != GSRT_OK) return s;
    FILE* f = std::fopen(path, "w");
    if (!f) return fail(ctx, GSRT_E_IO, std::string("cannot open ") + path);
    // the simulator's lines (gpu-sim.cc:1510-1518; any-hit rays: none, the Gaussian pipeline traces opaque)
    std::fprintf(f, "rt_num_hits = %llu\n", (unsigned long long)v[1]);
    std::fprintf(f, "rt_num_any_hits = 0\n");
    std::fprintf(f, "rt_n_anyhit_rays = 0\n");
    std::fprintf(f, "rt_n_closesthit_rays = %llu\n", (unsigned long long)v[0]);
    std::fprintf(f, "rt_n_total_rays = %llu\n", (unsigned long long)v[0]);
    std::fprintf(f, "rt_max_tree_depth = %llu\n", (unsigned long long)v[2]);
    std::fprintf(f, "rt_max_nodes_per_ray = %llu\n", (unsigned long long)v[3]);
    std::fprintf(f, "rt_tot_nodes_per_ray = %llu\n", (unsigned long long)v[4]);
    std::fprintf(f, "rt_avg_nodes_per_ray = %f\n", v[0] ? (float)v[4] / (float)v[0] : 0.0f);
    const bool ok = std::fclose(f) == 0;
    return ok ? GSRT_OK : fail(ctx, GSRT_E_IO, "write failed");
}

gsrt_status gsrt_last_stats(gsrt_ctx* ctx, uint64_t out[8], uint32_t* per_ray) {
    if (!ctx || !out) return GSRT_E_ARG;
    if (!ctx->last_stats) return fail(ctx, GSRT_E_STATE, "last render had no GSRT_FLAG_STATS");
    unsigned long long c[16];
    GSRT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    GSRT_HIP(ctx, hipMemcpy(c, ctx->d_counters, sizeof c, hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; ++i) out[i] = c[i];
    if (per_ray)
        GSRT_HIP(ctx, hipMemcpy(per_ray, ctx->d_ray_stats, 16ull * ctx->last_w * ctx->last_h, hipMemcpyDeviceToHost));
    return GSRT_OK;
}

}  // extern "C"
