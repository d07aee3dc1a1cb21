// gsrt_api_util.hpp -- what the C ABI's host files share (gsrt_api*.cpp, gsrt_trainer.cpp): pointer sides, a blocking
// call's staging and tail, the arrays of a model, and the one list of a call's arrays. Host only: no .hip file includes it.
#pragma once

#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "gsrt_internal.hpp"

namespace gsrt {

bool is_device_ptr(const void* p);

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
    char* take(size_t bytes) {
        char* p = base + used;
        used += unit(bytes);
        return p;
    }
};

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
gsrt_status finish_blocking(gsrt_ctx* ctx, gsrt_status s, const std::vector<Download>& downloads, void* const* tmp = nullptr);

// the arrays of a model in a fixed order with their floats per Gaussian (SH and features only when present)
struct ModelField {
    float* gsrt_model_arrays::*member;
    uint32_t floats;
};
uint32_t model_fields(const gsrt_model_arrays& m, ModelField out[6]);

// structs that must agree on sh, features and the channel count (a nullptr entry is an absent optional struct)
const char* check_model_sets(std::initializer_list<const gsrt_model_arrays*> sets, const gsrt_model_arrays& first);
const char* check_adam(const gsrt_adam_params* A);
// gsrt_frame_loss's refusals of its params struct (not NULL), under the caller's name (gsrt_api_model.cpp)
gsrt_status check_frame_loss_params(gsrt_ctx* ctx, const std::string& name, const gsrt_frame_loss_params& P);

// One array of a call: where its pointer stands (a variable of the call: a parameter, or a member of the call's own copy
// of a struct), its size, and whether the call reads and writes it. An absent optional array is a slot that holds
// nullptr. The list drives the side check and the blocking form's staging, and for the model calls the NULL and
// overlap checks.
struct CallArray {
    void* slot;  // a T**, of any T
    size_t bytes;
    bool in, out;
    template <class T>
    CallArray(T** slot_, size_t bytes_, bool in_, bool out_) : slot(slot_), bytes(bytes_), in(in_), out(out_) {}
    void* get() const {
        void* p;
        std::memcpy(&p, slot, sizeof p);
        return p;
    }
    void set(void* p) const { std::memcpy(slot, &p, sizeof p); }
};

void model_set_arrays(std::vector<CallArray>& list, gsrt_model_arrays& a, size_t n, bool in, bool out);

// where the present arrays of a call stand
enum class Side { host, device, mixed };
Side call_side(const std::vector<CallArray>& list);

// NULL arrays (n > 0), overlaps of a written array with any other (same: pairs of slots that may be one array), and the
// side, which must be one: 0 host, 1 device, -1 refused
int check_call_arrays(gsrt_ctx* ctx, const std::string& name, const std::vector<CallArray>& list, size_t n,
                      std::initializer_list<std::pair<const void*, const void*>> same);

// The blocking form. An array on the device is used in place; every host array gets a region of one device block (slots
// that hold the same host array share one) and its slot the region's address. Inputs are uploaded, `run` enqueues the
// kernels on the slots' pointers, then the downloads are queued: first `extra` (results that are no array of the call,
// read after `run`, which may fill it), then every host output's current byte count (`run` may lower one: rows that
// were not written stay as they were in the caller's array). The stream is drained and the block freed on every path.
gsrt_status run_staged(gsrt_ctx* ctx, const std::string& name, std::vector<CallArray>& list,
                       const std::function<gsrt_status()>& run, const std::vector<Download>* extra = nullptr);

}  // namespace gsrt
