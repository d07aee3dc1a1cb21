// gsrt_rng.hip -- counter-based normal noise on the device (gsrt_normal_noise) and its host hook (gsrt_debug_philox).
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): key = (seed lo, seed hi), block j
// has the counter (j lo, j hi, stream_id, 0). The four words of block j become out[4j .. 4j + 3] by two Box-Muller pairs
// in float32, every operation rounded on its own (the header writes the expressions down). A value is a pure function of
// (seed, stream_id, index): one lane owns one block whatever the grid, and a grid-stride loop covers counts beyond one
// grid. k_normal_noise is an HBM-bound streaming kernel: 16 B written per lane and nothing read, whole float4 stores where
// the base is 16-byte aligned, four dword stores otherwise; the last block's tail is cut by index. No LDS, no atomics.
#include <cstdint>

#include "gsrt_internal.hpp"

namespace gsrt {

struct PhiloxWords {
    uint32_t x[4];
};

__host__ __device__ inline void philox_mulhilo(uint32_t a, uint32_t b, uint32_t& hi, uint32_t& lo) {
    const uint64_t p = (uint64_t)a * (uint64_t)b;
    hi = (uint32_t)(p >> 32);
    lo = (uint32_t)p;
}

// Philox4x32-10 of Random123: ten rounds, the key bumped by the Weyl constants between them
__host__ __device__ inline PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                     uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        uint32_t hi0, lo0, hi1, lo1;
        philox_mulhilo(0xD2511F53u, c0, hi0, lo0);
        philox_mulhilo(0xCD9E8D57u, c2, hi1, lo1);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}

// one Box-Muller pair, the header's expressions in the header's order
__device__ inline void box_muller(uint32_t xa, uint32_t xb, float& z0, float& z1) {
    const float ua = ((float)(xa >> 8) + 0.5f) * 5.9604644775390625e-08f;  // 2^-24
    const float ub = ((float)(xb >> 8) + 0.5f) * 5.9604644775390625e-08f;
    const float r = sqrtf(-2.0f * logf(ua));
    const float th = 6.2831855f * ub;
    z0 = r * cosf(th);
    z1 = r * sinf(th);
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_normal_noise(uint64_t count, uint32_t k0, uint32_t k1, uint32_t stream_id,
                                                      float* __restrict__ out) {
    const uint64_t blocks = (count + 3) / 4;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x; j < blocks; j += stride) {
        const PhiloxWords w = philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), stream_id, 0u, k0, k1);
        float z[4];
        box_muller(w.x[0], w.x[1], z[0], z[1]);
        box_muller(w.x[2], w.x[3], z[2], z[3]);
        const uint64_t i = 4 * j;
        if (ALIGNED && i + 4 <= count) {
            *reinterpret_cast<float4*>(out + i) = make_float4(z[0], z[1], z[2], z[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < count) out[i + e] = z[e];
        }
    }
}

void launch_normal_noise(hipStream_t s, uint64_t count, uint64_t seed, uint32_t stream_id, float* out) {
    if (!count) return;
    const uint64_t blocks = (count + 3) / 4, groups = (blocks + 255) / 256;
    const uint32_t grid = (uint32_t)(groups < (1u << 20) ? groups : (1u << 20));  // beyond it the lanes stride
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (reinterpret_cast<uintptr_t>(out) % 16u == 0)
        hipLaunchKernelGGL(k_normal_noise<true>, dim3(grid), dim3(256), 0, s, count, k0, k1, stream_id, out);
    else
        hipLaunchKernelGGL(k_normal_noise<false>, dim3(grid), dim3(256), 0, s, count, k0, k1, stream_id, out);
}

}  // namespace gsrt

extern "C" gsrt_status gsrt_debug_philox(uint64_t seed, uint32_t stream_id, uint64_t first_block, uint64_t blocks,
                                         uint32_t* out) {
    if (!out && blocks) return GSRT_E_ARG;
    for (uint64_t b = 0; b < blocks; ++b) {
        const uint64_t j = first_block + b;
        const gsrt::PhiloxWords w =
            gsrt::philox4x32_10((uint32_t)j, (uint32_t)(j >> 32), stream_id, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
        for (int e = 0; e < 4; ++e) out[4 * b + e] = w.x[e];
    }
    return GSRT_OK;
}
