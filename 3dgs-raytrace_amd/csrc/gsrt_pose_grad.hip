// gsrt_pose_grad.hip -- the camera's gradient (gsrt_pose_grad): the splat rows of a gradient frame chained to the 16 floats
// of ubo.model_view, model_view_inverse held fixed. k_splat_grad_to_model's chain (gsrt_scene.hip) ended one step earlier,
// at the view-space position t = MV (c, 1) and the two Jacobian rows T0, T1, and summed over the Gaussians.
//
// Per valid Gaussian, in float32: cor_chain and cor_chain_grad (gsrt_project.hpp), the chain and backward
// k_splat_grad_to_model runs, give gt[0..3] = dL/dt (the (ppx, ppy) part through the general projection included; with
// DEPTH, gt[2] -= row[6]), g0[k] = dL/dT0[k], g1[k] = dL/dT1[k]. Its 16 contributions, in the ubo's column-major layout
// (entry c * 4 + r is row r, column c), with c4 = (centre, 1):
//     m[c * 4 + r] = gt[r] * c4[c]                                   t_r = sum_c MV[r][c] c4[c]
//     c < 3:  r = 0  + g0[c] * j00                                   T0[c] = j02 MV[2][c] + j00 MV[0][c]
//             r = 1  + g1[c] * j11                                   T1[c] = j12 MV[2][c] + j11 MV[1][c]
//             r = 2  + (g0[c] * j02 + g1[c] * j12)
// each rounded on its own. An invalid Gaussian (depth <= 0 or det <= 0) contributes nothing.
// The longest chain of rounded operations from the inputs to a contribution (the tests' N) ends in entry r = 2, c < 3:
// cor_chain_grad's 33 to gt[2] (DEPTH: 34), then gt[2] * c4[c] (1) and + the direct term (1), itself a shorter chain:
// 35 (DEPTH: 36).
//
// The sums over the Gaussians are taken in double, in an order that is a function of n alone:
//   k_pose_partial: workgroup b of 256 lanes owns the kPoseChunk consecutive Gaussians from b * kPoseChunk. Lane l adds
//     Gaussians b * kPoseChunk + j * 256 + l, j = 0, 1, .. (index order) into 16 doubles; the wave's lanes are combined
//     by a fixed xor butterfly (32, 16, .. 1), the workgroup's four waves through LDS in wave order, and the 16 doubles
//     go to partial[b].
//   k_pose_final: one workgroup of kPoseFinalLanes lanes. Lane l adds partials l, l + kPoseFinalLanes, .. in index order,
//     then the same butterfly and the waves in wave order; each sum is rounded to float once.
// No atomics, nothing depends on the grid's schedule: the same inputs give the same bits.
// A streaming kernel: 80 B read per Gaussian (48 B of parameters, 32 B of the row), nothing written but 128 B per chunk.
#include <cstdint>

#include "gsrt_internal.hpp"
#include "gsrt_project.hpp"

namespace gsrt {

constexpr uint32_t kPoseLanes = 256;
constexpr uint32_t kPosePerLane = kPoseChunk / kPoseLanes;
static_assert(kPoseChunk % kPoseLanes == 0 && kPoseFinalLanes % 64 == 0, "whole lanes, whole waves");

// the 16 contributions of one valid Gaussian (see the header), f its chain
template <bool DEPTH>
__device__ GSRT_INLINE void pose_terms(const gsrt_ubo& ubo, const gsrt_gauss_param& g, const CorChain& f,
                                       const float* __restrict__ row, float m[16]) {
    CorChainGrad d;
    cor_conic_grad(f, row, d);
    cor_chain_grad<DEPTH>(ubo, f, row, d);
    // t = MV c4, and T's own dependence on MV's 3x3
    const float c4[4] = {g.center_opacity[0], g.center_opacity[1], g.center_opacity[2], 1.0f};
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) m[c * 4 + r] = d.gt[r] * c4[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        m[c * 4 + 0] = m[c * 4 + 0] + d.g0[c] * f.j00;
        m[c * 4 + 1] = m[c * 4 + 1] + d.g1[c] * f.j11;
        m[c * 4 + 2] = m[c * 4 + 2] + (d.g0[c] * f.j02 + d.g1[c] * f.j12);
    }
}

// The 16 sums over the workgroup's lanes, in a fixed order: down each wave by the xor butterfly (every lane ends with
// the wave's sum, formed by the same tree), then the waves in wave order. Valid in lanes 0..15: lane k returns sum k.
// red: WAVES x 16 doubles of LDS.
template <uint32_t WAVES>
__device__ GSRT_INLINE double pose_block_sum(double acc[16], double (*red)[16]) {
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) red[wave][k] = acc[k];
    }
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x < 16) {
        s = red[0][threadIdx.x];
#pragma unroll
        for (uint32_t w = 1; w < WAVES; ++w) s += red[w][threadIdx.x];
    }
    return s;
}

template <bool DEPTH>
__global__ __launch_bounds__(kPoseLanes) void k_pose_partial(uint32_t n, const gsrt_ubo ubo,
                                                             const gsrt_gauss_param* __restrict__ params,
                                                             const float* __restrict__ rows, double* __restrict__ partial) {
    __shared__ double red[kPoseLanes / 64][16];
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
    const size_t base = (size_t)blockIdx.x * kPoseChunk + threadIdx.x;
    for (uint32_t j = 0; j < kPosePerLane; ++j) {
        const size_t i = base + (size_t)j * kPoseLanes;
        if (i >= n) break;
        const gsrt_gauss_param g = params[i];
        CorChain f;
        if (cor_chain(ubo, g, f) == kCorValid) {
            float m[16];
            pose_terms<DEPTH>(ubo, g, f, rows + 8 * i, m);
#pragma unroll
            for (int k = 0; k < 16; ++k) acc[k] += (double)m[k];
        }
    }
    const double s = pose_block_sum<kPoseLanes / 64>(acc, red);
    if (threadIdx.x < 16) partial[(size_t)blockIdx.x * 16 + threadIdx.x] = s;
}

__global__ __launch_bounds__(kPoseFinalLanes) void k_pose_final(uint32_t chunks, const double* __restrict__ partial,
                                                                float* __restrict__ out) {
    __shared__ double red[kPoseFinalLanes / 64][16];
    double acc[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] = 0.0;
    for (uint32_t p = threadIdx.x; p < chunks; p += kPoseFinalLanes) {
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[k] += partial[(size_t)p * 16 + k];
    }
    const double s = pose_block_sum<kPoseFinalLanes / 64>(acc, red);
    if (threadIdx.x < 16) out[threadIdx.x] = (float)s;
}

uint32_t pose_grad_chunks(uint32_t n) { return (uint32_t)(((uint64_t)n + kPoseChunk - 1) / kPoseChunk); }

void launch_pose_grad(hipStream_t s, uint32_t n, const gsrt_ubo& ubo, const gsrt_gauss_param* params, const float* rows,
                      bool depth, double* partial, float* out) {
    const uint32_t chunks = pose_grad_chunks(n);
    if (chunks) {
        const auto kernel = depth ? k_pose_partial<true> : k_pose_partial<false>;
        hipLaunchKernelGGL(kernel, dim3(chunks), dim3(kPoseLanes), 0, s, n, ubo, params, rows, partial);
    }
    hipLaunchKernelGGL(k_pose_final, dim3(1), dim3(kPoseFinalLanes), 0, s, chunks, partial, out);  // no chunks: 16 x +0
}

}  // namespace gsrt
