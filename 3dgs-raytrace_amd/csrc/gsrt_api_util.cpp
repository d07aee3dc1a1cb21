// gsrt_api_util.cpp -- the definitions of gsrt_api_util.hpp.
#include "gsrt_api_util.hpp"

namespace gsrt {

bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

gsrt_status finish_blocking(gsrt_ctx* ctx, gsrt_status s, const std::vector<Download>& downloads, void* const* tmp) {
    for (const Download& d : downloads)
        if (s == GSRT_OK && d.dst && hipMemcpyAsync(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
            s = fail(ctx, GSRT_E_DEVICE, d.what);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && s == GSRT_OK)
        s = fail(ctx, GSRT_E_DEVICE, std::string("render: ") + hipGetErrorString(hipGetLastError()));
    if (tmp) (void)hipFree(*tmp);
    if (s == GSRT_OK) s = check_error_word(ctx);
    return s;
}

uint32_t model_fields(const gsrt_model_arrays& m, ModelField out[6]) {
    uint32_t k = 0;
    out[k++] = {&gsrt_model_arrays::center, 3};
    out[k++] = {&gsrt_model_arrays::rot_rxyz, 4};
    out[k++] = {&gsrt_model_arrays::scale, 3};
    out[k++] = {&gsrt_model_arrays::opacity, 1};
    if (m.sh) out[k++] = {&gsrt_model_arrays::sh, 48};
    if (m.features) out[k++] = {&gsrt_model_arrays::features, m.feature_channels};
    return k;
}

const char* check_model_sets(std::initializer_list<const gsrt_model_arrays*> sets, const gsrt_model_arrays& first) {
    for (const gsrt_model_arrays* a : sets) {
        if (!a) continue;
        if (a->feature_channels > GSRT_MAX_FEATURES || (a->features == nullptr) != (a->feature_channels == 0))
            return "features need 1..GSRT_MAX_FEATURES channels, NULL exactly with 0 channels";
        if ((a->sh == nullptr) != (first.sh == nullptr) || a->feature_channels != first.feature_channels)
            return "the structs must agree on sh, features and feature_channels";
    }
    return nullptr;
}

const char* check_adam(const gsrt_adam_params* A) {
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

void model_set_arrays(std::vector<CallArray>& list, gsrt_model_arrays& a, size_t n, bool in, bool out) {
    ModelField f[6];
    const uint32_t nf = model_fields(a, f);
    for (uint32_t i = 0; i < nf; ++i) list.push_back({&(a.*f[i].member), sizeof(float) * f[i].floats * n, in, out});
}

Side call_side(const std::vector<CallArray>& list) {
    size_t given = 0, on_dev = 0;
    for (const CallArray& a : list)
        if (const void* p = a.get()) {
            ++given;
            if (is_device_ptr(p)) ++on_dev;
        }
    return !on_dev ? Side::host : on_dev == given ? Side::device : Side::mixed;
}

int check_call_arrays(gsrt_ctx* ctx, const std::string& name, const std::vector<CallArray>& list, size_t n,
                      std::initializer_list<std::pair<const void*, const void*>> same) {
    if (!n) return 1;
    for (const CallArray& a : list)
        if (!a.get()) return fail(ctx, GSRT_E_ARG, name + "a NULL array"), -1;
    for (size_t i = 0; i < list.size(); ++i)
        for (size_t j = i + 1; j < list.size(); ++j) {
            if (!list[i].out && !list[j].out) continue;
            const uintptr_t a = reinterpret_cast<uintptr_t>(list[i].get()), b = reinterpret_cast<uintptr_t>(list[j].get());
            if (!(a < b + list[j].bytes && b < a + list[i].bytes)) continue;
            bool allowed = false;
            for (const auto& p : same)
                if (a == b && ((p.first == list[i].slot && p.second == list[j].slot) ||
                               (p.first == list[j].slot && p.second == list[i].slot)))
                    allowed = true;
            if (!allowed) return fail(ctx, GSRT_E_ARG, name + "an output array overlaps another array of the call"), -1;
        }
    const Side side = call_side(list);
    if (side == Side::mixed)
        return fail(ctx, GSRT_E_ARG, name + "the arrays must all be host pointers or all be device pointers"), -1;
    return side == Side::device ? 1 : 0;
}

gsrt_status run_staged(gsrt_ctx* ctx, const std::string& name, std::vector<CallArray>& list,
                       const std::function<gsrt_status()>& run, const std::vector<Download>* extra) {
    std::vector<void*> host(list.size(), nullptr);  // nullptr: absent or on the device
    std::vector<char*> dev(list.size(), nullptr);
    bool any = false;
    size_t bytes = 0;
    for (size_t i = 0; i < list.size(); ++i) {
        void* const p = list[i].get();
        if (!p || is_device_ptr(p)) continue;
        host[i] = p;
        bool shared = false;
        for (size_t j = 0; j < i; ++j) shared = shared || host[j] == p;
        if (!shared) bytes += Staging::unit(list[i].bytes);
        any = true;
    }
    Staging tmp;
    if (any) GSRT_HIP(ctx, hipMalloc(&tmp.base, bytes ? bytes : 16));
    void* const tmpv = tmp.base;
    gsrt_status s = GSRT_OK;
    for (size_t i = 0; i < list.size(); ++i) {
        if (!host[i]) continue;
        for (size_t j = 0; j < i; ++j)
            if (host[j] == host[i]) dev[i] = dev[j];
        if (!dev[i]) {
            dev[i] = tmp.take(list[i].bytes);
            if (list[i].in && s == GSRT_OK && list[i].bytes &&
                hipMemcpyAsync(dev[i], host[i], list[i].bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
                s = fail(ctx, GSRT_E_DEVICE, name + "upload failed");
        }
        list[i].set(dev[i]);
    }
    if (s == GSRT_OK) s = run();
    const std::string what = name + "download failed";
    std::vector<Download> downloads;
    if (extra) downloads = *extra;
    for (size_t i = 0; i < list.size(); ++i)
        if (host[i] && list[i].out && list[i].bytes) downloads.push_back({host[i], dev[i], list[i].bytes, what.c_str()});
    return finish_blocking(ctx, s, downloads, &tmpv);
}

}  // namespace gsrt
