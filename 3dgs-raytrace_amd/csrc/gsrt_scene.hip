// gsrt_scene.hip -- per-Gaussian kernels: scene build (a1) and per-frame projection (rint:62-102).
//
// Both are one thread per Gaussian, HBM-bound streaming kernels: 40 B in / 72 B out for the scene
// build, 72 B in / 64 B out per frame for the projection.
#include <algorithm>
#include <cstdint>

#include "gsrt_cov3d.hpp"
#include "gsrt_internal.hpp"
#include "gsrt_project.hpp"

namespace gsrt {

// Gauss::init_cov3d / init_radius / BoundingBox (RayTracingInVulkan/src/Assets/Sphere.hpp:108-165),
// packed as Scene.cpp:125-136 does: cov3d_pack (gsrt_cov3d.hpp) per Gaussian.
__global__ __launch_bounds__(256) void k_cov3d(uint32_t n, const float* __restrict__ center,
                                               const float* __restrict__ rot, const float* __restrict__ scale,
                                               const float* __restrict__ opacity, gsrt_gauss_param* __restrict__ params,
                                               gsrt_aabb* __restrict__ aabbs) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float r = rot[4 * i + 0], x = rot[4 * i + 1], y = rot[4 * i + 2], z = rot[4 * i + 3];
    const float s0 = scale[3 * i + 0], s1 = scale[3 * i + 1], s2 = scale[3 * i + 2];
    const float c[3] = {center[3 * i + 0], center[3 * i + 1], center[3 * i + 2]};
    gsrt_gauss_param g;
    gsrt_aabb a;
    cov3d_pack(c, r, x, y, z, s0, s1, s2, opacity[i], g, a);  // gsrt_cov3d.hpp: shared with the model step
    params[i] = g;
    aabbs[i] = a;
}

void launch_cov3d(hipStream_t s, uint32_t n, const float* center, const float* rot, const float* scale,
                  const float* opacity, gsrt_gauss_param* params, gsrt_aabb* aabbs) {
    if (!n) return;
    hipLaunchKernelGGL(k_cov3d, dim3((n + 255) / 256), dim3(256), 0, s, n, center, rot, scale, opacity, params, aabbs);
}

// keyed (per frame slot, one bit per splat, nullable): bit 0 = the splat's record depth and node key in this slot
// are +inf (it was outside the rank's tiles when the slot was last projected), so while it stays outside, nothing
// needs writing. Bits are rewritten here every projection; all ones (unknown) after a build, a buffer allocation,
// or a frame that wrote the slot without this kernel's bookkeeping (launch_render).
template <int MODE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6))) void k_project(uint32_t n, const gsrt_ubo ubo,
                                                 const gsrt_gauss_param* __restrict__ params,
                                                 const gsrt_aabb* __restrict__ aabbs, SplatRec* __restrict__ recs,
                                                 BvhNode* __restrict__ nodes, const uint32_t* __restrict__ gid_slot,
                                                 float4* __restrict__ footprint,
                                                 unsigned long long* __restrict__ counters, const RankTiles own,
                                                 uint32_t* __restrict__ keyed, uint32_t leaf_fp,
                                                 uint32_t* __restrict__ depth_unsafe) {
    __builtin_amdgcn_s_setprio(kPrepSetprio);  // see gsrt_render.hip: ahead of the render kernel's waves
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    // the frame's stats words (ordered before every kernel that adds to them); the error word stays: a pipelined
    // frame's projection runs while the previous frame's render may still set it
    if (i < kCounters && i != kErrWord) counters[i] = 0;
    bool k = true;
    if (i < n) {
        const bool prev = keyed ? ((keyed[i >> 5] >> (i & 31u)) & 1u) != 0 : true;
        k = project_one<MODE>(i, n, ubo, params, aabbs, recs, nodes, gid_slot, footprint, own, prev, leaf_fp != 0,
                              depth_unsafe);
    }
    if (keyed) {  // one-wave workgroups: lanes 0 and 32 write the wave's two bitmap words
        const uint64_t m = __ballot(k);
        if ((threadIdx.x & 31u) == 0 && i < n) keyed[i >> 5] = (uint32_t)(m >> (threadIdx.x & 32u));
    }
}

void launch_project(hipStream_t st, uint32_t n, uint32_t mode, const gsrt_ubo& ubo, const gsrt_gauss_param* params,
                    const gsrt_aabb* aabbs, SplatRec* recs, BvhNode* nodes, const uint32_t* gid_slot, float4* footprint,
                    unsigned long long* counters, const RankTiles* own, uint32_t* keyed, bool leaf_fp,
                    uint32_t* depth_unsafe) {
    const RankTiles all{};  // active = 0: every splat kept
    if (!n) {
        (void)hipMemsetAsync(counters, 0, sizeof(unsigned long long) * kErrWord, st);
        (void)hipMemsetAsync(counters + kErrWord + 1, 0, sizeof(unsigned long long) * (kCounters - kErrWord - 1), st);
        return;
    }
    dim3 grid((n + 63) / 64), block(64);
    if (n < 2) nodes = nullptr;  // a single Gaussian is the root leaf: no parent node to hold its key
    if ((mode & 0xff) == GSRT_MODE_REF)
        hipLaunchKernelGGL(k_project<GSRT_MODE_REF>, grid, block, 0, st, n, ubo, params, aabbs, recs, nullptr, nullptr,
                           nullptr, counters, all, nullptr, 0u, nullptr);
    else hipLaunchKernelGGL(k_project<GSRT_MODE_COR>, grid, block, 0, st, n, ubo, params, aabbs, recs, nodes, gid_slot,
                            footprint, counters, own && footprint ? *own : all, keyed, leaf_fp && nodes ? 1u : 0u,
                            depth_unsafe);
}

// cor_chain backwards to the model (gsrt_splat_grad_to_model): one lane per Gaussian takes its splat row
// (gsrt_render_splat_grad: dL/d(ppx, ppy, A, B, C) in slots 0..4) to dL/d(centre) and dL/d(cov3d). cor_chain recomputes the
// forward's float32 intermediates, cor_conic_grad and cor_chain_grad (gsrt_project.hpp) take the row to W = dL/dV and
// dL/dt; this kernel's own part:
//   dL/dSigma = T^T W T (an off-diagonal cov3d entry stands twice in Sigma: twice the matrix entry),
//   dL/d(centre) = MV^T dL/dt.
// An invalid splat (depth <= 0 or det <= 0) gets +0, and so does a valid one whose row is all +0 (no ray reached it): a
// zero is written as +0. No atomics.
// The longest chain of rounded operations from the inputs to an output (the tests' N) ends in a centre entry:
// cor_chain_grad's 33 to dL/dt, then MV^T dL/dt (4): 37.
// DEPTH (the second instantiation, gsrt_splat_depth_grad_to_model): the row is gsrt_render_splat_depth_grad's, whose
// slot 6 holds dL/d(depth): cor_chain_grad's 34, then the same 4: 38. Without DEPTH slot 6 is never read. Nothing of it
// reaches cov3d.
// Not a prep kernel: ordinary priority, 256 lanes a workgroup as the scene build's kernels.
template <bool DEPTH>
__global__ __launch_bounds__(256) void k_splat_grad_to_model(uint32_t n, const gsrt_ubo ubo,
                                                             const gsrt_gauss_param* __restrict__ params,
                                                             const float* __restrict__ rows, float* __restrict__ grad_center,
                                                             float* __restrict__ grad_cov, uint32_t accumulate) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const gsrt_gauss_param g = params[i];
    const float* row = rows + 8 * (size_t)i;
    float dc[3] = {0.0f, 0.0f, 0.0f}, dS[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    CorChain f;
    if (cor_chain(ubo, g, f) == kCorValid) {
        CorChainGrad d;
        cor_conic_grad(f, row, d);
        // dL/dSigma = T^T W T, entries in cov3d's order
        const float *T0 = f.T0, *T1 = f.T1;
        int e = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = a; b < 3; ++b) {
                const float s = (d.w00 * (T0[a] * T0[b]) + d.w01 * (T0[a] * T1[b] + T1[a] * T0[b])) + d.w11 * (T1[a] * T1[b]);
                dS[e++] = a == b ? s : 2.0f * s;
            }
        cor_chain_grad<DEPTH>(ubo, f, row, d);
        const float* MV = ubo.model_view;
        const float* gt = d.gt;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            dc[k] = ((cm(MV, k, 0) * gt[0] + cm(MV, k, 1) * gt[1]) + cm(MV, k, 2) * gt[2]) + cm(MV, k, 3) * gt[3];
    }
    float* oc = grad_center + 3 * (size_t)i;
    float* ov = grad_cov + 6 * (size_t)i;
    // + 0.0f: a zero result is written as +0 whatever the signs of its terms. A valid Gaussian that no ray reached has a
    // row of +0, W = -Q G Q of it is -0, and sums of products with it come out as -0 wherever every term is negative.
#pragma unroll
    for (int k = 0; k < 3; ++k) oc[k] = accumulate ? oc[k] + dc[k] : dc[k] + 0.0f;
#pragma unroll
    for (int k = 0; k < 6; ++k) ov[k] = accumulate ? ov[k] + dS[k] : dS[k] + 0.0f;
}

void launch_splat_grad_to_model(hipStream_t s, uint32_t n, const gsrt_ubo& ubo, const gsrt_gauss_param* params,
                                const float* rows, float* grad_center, float* grad_cov, bool accumulate, bool depth) {
    if (!n) return;
    const auto kernel = depth ? k_splat_grad_to_model<true> : k_splat_grad_to_model<false>;
    hipLaunchKernelGGL(kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, ubo, params, rows, grad_center, grad_cov,
                       accumulate ? 1u : 0u);
}

// Scene-update copies (gsrt_scene_update / refit / stream_pages from device sources) beside the previous frames'
// kernels: 1024 one-wave workgroups looping over the rows, each copying 4 x 1 KB per step (16 B per lane in flight 4
// times). Few short workgroups of few VGPRs take the slots render waves free without crowding them out. Measured alone
// on 240 MB (profiles/probes/copy_probe.hip): 2.51 TB/s read + write; one pass with a workgroup per 4 KB reached 4.99
// and 16384 looping workgroups 4.71, but both were slower beside the render kernel on the C5 share; the
// runtime's blit (5.32 alone) took 2.9 ms for C5's 360 MB beside a running render kernel (starved of dispatch slots)
constexpr uint32_t kCopyUnroll = 4;
constexpr size_t kCopyGroups = 1024;
__global__ __launch_bounds__(64) void k_copy_rows(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n16) {
    __builtin_amdgcn_s_setprio(kPrepSetprio);
    const size_t stride = (size_t)gridDim.x * (64 * kCopyUnroll);
    for (size_t base = (size_t)blockIdx.x * (64 * kCopyUnroll) + threadIdx.x; base < n16; base += stride) {
        uint4 v[kCopyUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kCopyUnroll; ++u)
            if (base + 64 * u < n16) v[u] = src[base + 64 * u];
#pragma unroll
        for (uint32_t u = 0; u < kCopyUnroll; ++u)
            if (base + 64 * u < n16) dst[base + 64 * u] = v[u];
    }
}

void launch_copy_d2d(hipStream_t s, void* dst, const void* src, size_t bytes) {
    if (!bytes) return;
    if (((uintptr_t)dst | (uintptr_t)src | bytes) & 15u) {
        (void)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s);
        return;
    }
    const size_t n16 = bytes / 16;
    const size_t blocks = std::min(kCopyGroups, (n16 + 64 * kCopyUnroll - 1) / (64 * kCopyUnroll));
    hipLaunchKernelGGL(k_copy_rows, dim3((uint32_t)blocks), dim3(64), 0, s, reinterpret_cast<uint4*>(dst),
                       reinterpret_cast<const uint4*>(src), n16);
}

// Feature rows of a device source (gsrt_scene_set_features): one thread per float of the padded table, so that a row
// is 64 B at a 64-B multiple, which the render kernel's stage DMA fetches as four 16-B pieces
__global__ __launch_bounds__(256) void k_pad_features(float* __restrict__ rows, const float* __restrict__ src, size_t n16,
                                                      uint32_t channels) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n16) return;
    const uint32_t k = (uint32_t)(i & 15u);
    rows[i] = k < channels ? src[(i >> 4) * channels + k] : 0.0f;
}

void launch_pad_features(hipStream_t s, float* rows, const float* src, uint32_t n, uint32_t channels) {
    const size_t n16 = (size_t)n * 16;
    if (!n16) return;
    hipLaunchKernelGGL(k_pad_features, dim3((uint32_t)((n16 + 255) / 256)), dim3(256), 0, s, rows, src, n16, channels);
}

// Gradient rows of a gradient frame (gsrt_render_feature_grad) to the caller's table: one thread per output float,
// dst[g][c] = rows[g][c] of the 64-B rows the render kernel added to, or dst[g][c] += it when accumulate
__global__ __launch_bounds__(256) void k_grad_compact(float* __restrict__ dst, const float* __restrict__ rows, size_t nc,
                                                      uint32_t channels, uint32_t accumulate) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nc) return;
    const size_t g = i / channels;
    const float v = rows[g * 16 + (i - g * channels)];
    dst[i] = accumulate ? dst[i] + v : v;
}

void launch_grad_compact(hipStream_t s, float* dst, const float* rows, uint32_t n, uint32_t channels, bool accumulate) {
    const size_t nc = (size_t)n * channels;
    if (!nc) return;
    hipLaunchKernelGGL(k_grad_compact, dim3((uint32_t)((nc + 255) / 256)), dim3(256), 0, s, dst, rows, nc, channels,
                       accumulate ? 1u : 0u);
}

// SH rows of a device source (gsrt_scene_set_sh): one thread per float of the device layout [gauss][rgb][coef], read from
// the API layout [gauss][coef][rgb]; word 0 of a channel is (s_0 Y_0) + 0.5, the product rounded before the sum, as
// upload_common computes it on the host (the library is built with -ffp-contract=off)
__global__ __launch_bounds__(256) void k_sh_rows(float* __restrict__ rows, const float* __restrict__ src, size_t n48) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n48) return;
    const size_t g = i / 48;
    const uint32_t r = (uint32_t)(i - g * 48), c = r >> 4, k = r & 15u;
    const float s = src[g * 48 + 3 * k + c];
    rows[i] = k == 0 ? __fadd_rn(__fmul_rn(s, kShY0), 0.5f) : s;
}

void launch_sh_rows(hipStream_t s, float* rows, const float* src, uint32_t n) {
    const size_t n48 = (size_t)n * 48;
    if (!n48) return;
    hipLaunchKernelGGL(k_sh_rows, dim3((uint32_t)((n48 + 255) / 256)), dim3(256), 0, s, rows, src, n48);
}

// SH gradient rows of an SH gradient frame (gsrt_render_sh_grad) to the caller's table: one thread per output float,
// dst[g][coef][rgb] = rows[g][rgb][coef] of the 192-B rows the render kernel added to, or += when accumulate
__global__ __launch_bounds__(256) void k_sh_grad_compact(float* __restrict__ dst, const float* __restrict__ rows, size_t n48,
                                                         uint32_t accumulate) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n48) return;
    const size_t g = i / 48;
    const uint32_t r = (uint32_t)(i - g * 48), k = r / 3, c = r - 3 * k;
    const float v = rows[g * 48 + 16 * c + k];
    dst[i] = accumulate ? dst[i] + v : v;
}

void launch_sh_grad_compact(hipStream_t s, float* dst, const float* rows, uint32_t n, bool accumulate) {
    const size_t n48 = (size_t)n * 48;
    if (!n48) return;
    hipLaunchKernelGGL(k_sh_grad_compact, dim3((uint32_t)((n48 + 255) / 256)), dim3(256), 0, s, dst, rows, n48,
                       accumulate ? 1u : 0u);
}

}  // namespace gsrt
