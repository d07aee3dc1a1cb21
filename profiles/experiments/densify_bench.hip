// densify_bench.hip -- the densify pass at the benchmark's size against a device-to-device copy of the same traffic, and
// against a write kernel whose SH rows move one lane per row (the variant the library does not keep).
//
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -fhip-fp32-correctly-rounded-divide-sqrt \
//         -o densify_bench profiles/experiments/densify_bench.hip && ./densify_bench [n]
//
// The library's kernels are compiled in from its own source (count, scan, write: exactly what gsrt_densify_async enqueues);
// k_densify_write_lane_rows is k_densify_write with the cooperative SH copy replaced. 1M Gaussians with SH rows, 10 % split,
// 10 % clone, 10 % prune. HIP events on one stream, 5 warm-up rounds, 30 timed rounds with the three alternating; medians.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../3dgs-raytrace_amd/csrc/gsrt_densify.hip"

namespace gsrt {
__global__ __launch_bounds__(kDensBlock) void k_densify_write_lane_rows(uint32_t n, const gsrt_densify_params P,
                                                                        const gsrt_model_arrays in,
                                                                        const float* __restrict__ stats,
                                                                        const float* __restrict__ noise,
                                                                        const gsrt_model_arrays out,
                                                                        int32_t* __restrict__ origin, uint32_t cap,
                                                                        const uint32_t* __restrict__ block_base,
                                                                        const uint32_t* __restrict__ n_out) {
    __shared__ uint32_t wsum[kDensWaves];
    const uint32_t total = *n_out;
    if (total > cap || total > GSRT_MAX_GAUSSIANS) return;
    const uint32_t t = threadIdx.x, g = blockIdx.x * kDensBlock + t;
    bool split = false;
    const uint32_t c = g < n ? densify_rows(P, in.scale, in.opacity, stats, g, split) : 0u;
    const uint64_t m1 = __ballot(c >= 1u), m2 = __ballot(c == 2u);
    const uint32_t wave = t >> 6;
    if ((t & 63u) == 0) wsum[wave] = (uint32_t)(__popcll(m1) + __popcll(m2));
    __syncthreads();
    uint32_t local = dens_popc_below(m1) + dens_popc_below(m2);
    for (uint32_t w = 0; w < wave; ++w) local += wsum[w];
    if (!c) return;
    const size_t o0 = (size_t)block_base[blockIdx.x] + local;
    const float r = in.rot_rxyz[4 * (size_t)g], x = in.rot_rxyz[4 * (size_t)g + 1], y = in.rot_rxyz[4 * (size_t)g + 2],
                z = in.rot_rxyz[4 * (size_t)g + 3];
    const float Rc[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                         2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                         2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)};
    for (uint32_t k = 0; k < c; ++k) {
        const size_t o = o0 + k;
        for (int j = 0; j < 3; ++j) {
            float cj = in.center[3 * (size_t)g + j], sj = in.scale[3 * (size_t)g + j];
            if (split) {
                const float* zn = noise + 6 * (size_t)g + 3 * k;
                const float v0 = in.scale[3 * (size_t)g] * zn[0], v1 = in.scale[3 * (size_t)g + 1] * zn[1],
                            v2 = in.scale[3 * (size_t)g + 2] * zn[2];
                cj = cj + ((v0 * Rc[j * 3 + 0] + v1 * Rc[j * 3 + 1]) + v2 * Rc[j * 3 + 2]);
                sj = sj / P.shrink;
            }
            out.center[3 * o + j] = cj;
            out.scale[3 * o + j] = sj;
        }
        out.rot_rxyz[4 * o] = r; out.rot_rxyz[4 * o + 1] = x; out.rot_rxyz[4 * o + 2] = y; out.rot_rxyz[4 * o + 3] = z;
        out.opacity[o] = in.opacity[g];
        origin[o] = (split || k) ? -1 - (int32_t)g : (int32_t)g;
        // the variant: this lane walks the whole 192-byte row
        const uint4* s = reinterpret_cast<const uint4*>(in.sh) + (size_t)g * kShPieces;
        uint4* d = reinterpret_cast<uint4*>(out.sh) + o * kShPieces;
#pragma unroll
        for (uint32_t p = 0; p < kShPieces; ++p) d[p] = s[p];
    }
}
}  // namespace gsrt

#define CK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(_e)); return 1; } } while (0)

int main(int argc, char** argv) {
    const uint32_t n = argc > 1 ? (uint32_t)std::atol(argv[1]) : 1000000u;
    const uint32_t cap = 2 * n;
    std::vector<float> center(3ull * n), rot(4ull * n), scale(3ull * n), opacity(n), sh(48ull * n), stats(2ull * n), noise(6ull * n);
    uint64_t state = 12345;
    auto rnd = [&] { state = state * 6364136223846793005ull + 1442695040888963407ull; return (float)((state >> 40) & 0xffffff) / 16777216.0f; };
    size_t splits = 0, clones = 0, prunes = 0;
    for (uint32_t g = 0; g < n; ++g) {
        const float u = rnd();
        for (int j = 0; j < 3; ++j) center[3ull * g + j] = rnd() * 10.0f - 5.0f;
        rot[4ull * g] = 0.8f; rot[4ull * g + 1] = 0.2f; rot[4ull * g + 2] = -0.4f; rot[4ull * g + 3] = 0.4f;
        const bool split = u >= 0.1f && u < 0.2f, clone = u >= 0.2f && u < 0.3f, prune = u < 0.1f;
        for (int j = 0; j < 3; ++j) scale[3ull * g + j] = (split ? 0.5f : 0.01f) + 0.04f * rnd();
        opacity[g] = prune ? 0.001f : 0.5f;
        stats[2ull * g] = (split || clone) ? 3.0f : 0.0003f;
        stats[2ull * g + 1] = 3.0f;
        for (int j = 0; j < 6; ++j) noise[6ull * g + j] = rnd() - 0.5f;
        for (int j = 0; j < 48; ++j) sh[48ull * g + j] = rnd();
        splits += split; clones += clone; prunes += prune;
    }
    const gsrt_densify_params P{0.5f, 0.25f, 0.005f, 0.0f, 1.6f, {0, 0, 0}};
    const size_t rows_out = n - prunes + splits + clones;
    gsrt_model_arrays in{}, out[2] = {};
    float *d_stats, *d_noise;
    int32_t* d_origin[2];
    uint32_t *d_ws, *d_n;
    auto up = [&](float** d, const std::vector<float>& h) {
        if (hipMalloc(d, h.size() * 4) != hipSuccess) return false;
        return hipMemcpy(*d, h.data(), h.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    };
    if (!up(&in.center, center) || !up(&in.rot_rxyz, rot) || !up(&in.scale, scale) || !up(&in.opacity, opacity) ||
        !up(&in.sh, sh) || !up(&d_stats, stats) || !up(&d_noise, noise)) return 1;
    for (int v = 0; v < 2; ++v) {
        CK(hipMalloc(&out[v].center, 12ull * cap)); CK(hipMalloc(&out[v].rot_rxyz, 16ull * cap));
        CK(hipMalloc(&out[v].scale, 12ull * cap)); CK(hipMalloc(&out[v].opacity, 4ull * cap));
        CK(hipMalloc(&out[v].sh, 192ull * cap)); CK(hipMalloc(&d_origin[v], 4ull * cap));
    }
    const uint32_t nblocks = gsrt::densify_blocks(n);
    CK(hipMalloc(&d_ws, 4ull * (nblocks + 1)));
    d_n = d_ws + nblocks;
    // the traffic of the pass: what its kernels read plus what they write
    const double read_b = 24.0 * n + 24.0 * n + 44.0 * (n - prunes) + 24.0 * splits + 192.0 * rows_out;
    const double write_b = (44.0 + 4.0 + 192.0) * rows_out + 4.0 * nblocks;
    const size_t copy_b = (size_t)((read_b + write_b) / 2.0) & ~(size_t)15;
    char *d_a, *d_b;
    CK(hipMalloc(&d_a, copy_b)); CK(hipMalloc(&d_b, copy_b));
    CK(hipMemset(d_a, 1, copy_b));
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    hipEvent_t e[6];
    for (auto& x : e) CK(hipEventCreate(&x));
    std::vector<float> t_coop, t_lane, t_copy, t_wcoop, t_wlane;
    for (int it = 0; it < 35; ++it) {
        CK(hipEventRecord(e[0], st));
        gsrt::launch_densify_count(st, n, P, in.scale, in.opacity, d_stats, d_ws, d_n);
        CK(hipEventRecord(e[1], st));
        gsrt::launch_densify_write(st, n, P, in, d_stats, d_noise, out[0], d_origin[0], cap, d_ws, d_n);
        CK(hipEventRecord(e[2], st));
        gsrt::launch_densify_count(st, n, P, in.scale, in.opacity, d_stats, d_ws, d_n);
        CK(hipEventRecord(e[3], st));
        hipLaunchKernelGGL(gsrt::k_densify_write_lane_rows, dim3(nblocks), dim3(gsrt::kDensBlock), 0, st, n, P, in, d_stats,
                           d_noise, out[1], d_origin[1], cap, d_ws, d_n);
        CK(hipEventRecord(e[4], st));
        CK(hipMemcpyAsync(d_b, d_a, copy_b, hipMemcpyDeviceToDevice, st));
        CK(hipEventRecord(e[5], st));
        CK(hipStreamSynchronize(st));
        if (it < 5) continue;
        float ms[5];
        for (int k = 0; k < 5; ++k) CK(hipEventElapsedTime(&ms[k], e[k], e[k + 1]));
        t_coop.push_back(ms[0] + ms[1]); t_wcoop.push_back(ms[1]);
        t_lane.push_back(ms[2] + ms[3]); t_wlane.push_back(ms[3]);
        t_copy.push_back(ms[4]);
    }
    // the two variants wrote the same model
    uint32_t got = 0;
    CK(hipMemcpy(&got, d_n, 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> a(48ull * got), b(48ull * got);
    CK(hipMemcpy(a.data(), out[0].sh, 192ull * got, hipMemcpyDeviceToHost));
    CK(hipMemcpy(b.data(), out[1].sh, 192ull * got, hipMemcpyDeviceToHost));
    std::vector<uint32_t> ca(3ull * got), cb(3ull * got);
    CK(hipMemcpy(ca.data(), out[0].center, 12ull * got, hipMemcpyDeviceToHost));
    CK(hipMemcpy(cb.data(), out[1].center, 12ull * got, hipMemcpyDeviceToHost));
    const bool same = got == rows_out && a == b && ca == cb;
    auto med = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    auto lo = [](const std::vector<float>& v) { return *std::min_element(v.begin(), v.end()); };
    auto hi = [](const std::vector<float>& v) { return *std::max_element(v.begin(), v.end()); };
    const double gb = (read_b + write_b) / 1e9;
    std::printf("n %u  rows out %zu  split %zu  clone %zu  prune %zu  variants agree %d\n", n, rows_out, splits, clones, prunes, (int)same);
    std::printf("traffic of the pass %.1f MB (read %.1f + written %.1f); copy of %.1f MB (read + written the same total)\n",
                gb * 1e3, read_b / 1e6, write_b / 1e6, copy_b / 1e6);
    std::printf("densify pass, cooperative SH rows : median %.4f ms (min %.4f max %.4f)  %.0f GB/s   write kernel alone %.4f ms\n",
                med(t_coop), lo(t_coop), hi(t_coop), gb / (med(t_coop) * 1e-3), med(t_wcoop));
    std::printf("densify pass, lane-per-row SH rows: median %.4f ms (min %.4f max %.4f)  %.0f GB/s   write kernel alone %.4f ms\n",
                med(t_lane), lo(t_lane), hi(t_lane), gb / (med(t_lane) * 1e-3), med(t_wlane));
    std::printf("hipMemcpyAsync device to device   : median %.4f ms (min %.4f max %.4f)  %.0f GB/s\n", med(t_copy), lo(t_copy),
                hi(t_copy), 2.0 * copy_b / 1e9 / (med(t_copy) * 1e-3));
    return same ? 0 : 2;
}
