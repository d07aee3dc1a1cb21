// gsrt_pose_grad.hip -- the camera's gradient (gsrt_pose_grad): the splat rows of a gradient frame chained to the 16 floats
// of ubo.model_view, model_view_inverse held fixed. k_splat_grad_to_model's chain (gsrt_scene.hip) ended one step earlier,
// at the view-space position t = MV (c, 1) and the two Jacobian rows T0, T1, and summed over the Gaussians.
//
// Per valid Gaussian, in float32 with k_splat_grad_to_model's own operations in its own order (restated here, so that
// kernel's outputs stay what they are): gt[0..3] = dL/dt (the (ppx, ppy) part through the general projection included; with
// DEPTH, gt[2] -= row[6]), g0[k] = dL/dT0[k], g1[k] = dL/dT1[k]. Its 16 contributions, in the ubo's column-major layout
// (entry c * 4 + r is row r, column c), with c4 = (centre, 1):
//     m[c * 4 + r] = gt[r] * c4[c]                                   t_r = sum_c MV[r][c] c4[c]
//     c < 3:  r = 0  + g0[c] * j00                                   T0[c] = j02 MV[2][c] + j00 MV[0][c]
//             r = 1  + g1[c] * j11                                   T1[c] = j12 MV[2][c] + j11 MV[1][c]
//             r = 2  + (g0[c] * j02 + g1[c] * j12)
// each rounded on its own. An invalid Gaussian (depth <= 0 or det <= 0) contributes nothing.
// The longest chain of rounded operations from the inputs to a contribution (the tests' N) ends in entry r = 2, c < 3 by
// way of the conic: t (4), id (1), id^2 (1), j02 (1), T0 (1), u0 (3), v00 (4), det (1), 1 / det (1), A (1), Q G (2), W (2),
// dL/dT0 (2), dL/dj02 (3), dL/d(id) (4), dL/dt2 (1), + the ppx, ppy part (1): 33 so far, k_splat_grad_to_model's 37 less
// its final MV^T dL/dt (4); then gt[2] * c4[c] (1) and + the direct term (1), itself a shorter chain: 35. DEPTH: one more,
// gt[2] - row[6], before the product: 36.
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

namespace gsrt {

constexpr uint32_t kPoseLanes = 256;
constexpr uint32_t kPosePerLane = kPoseChunk / kPoseLanes;
static_assert(kPoseChunk % kPoseLanes == 0 && kPoseFinalLanes % 64 == 0, "whole lanes, whole waves");

// the 16 contributions of one Gaussian (see the header); false, and m untouched, for an invalid one
template <bool DEPTH>
__device__ GSRT_INLINE bool pose_terms(const gsrt_ubo& ubo, const gsrt_gauss_param& g, const float* __restrict__ row,
                                       float m[16]) {
    const float4 r0 = make_float4(row[0], row[1], row[2], row[3]);  // dppx, dppy, dA, dB
    const float gC = row[4];
    const float* MV = ubo.model_view;
    const float* P = ubo.projection;
    const float c4[4] = {g.center_opacity[0], g.center_opacity[1], g.center_opacity[2], 1.0f};
    float t[4];
    mul4v(MV, c4, t);
    const float depth = -t[2];
    if (!(depth > 0.0f)) return false;
    float ph[4];
    mul4v(P, t, ph);
    const float fx = (cm(P, 0, 0) * (float)ubo.width) * 0.5f;
    const float fy = (cm(P, 1, 1) * (float)ubo.height) * 0.5f;
    const float id = 1.0f / depth;
    const float id2 = id * id;
    const float fxt0 = fx * t[0], fyt1 = fy * t[1];
    const float j00 = fx * id, j02 = fxt0 * id2, j11 = fy * id, j12 = fyt1 * id2;
    float T0[3], T1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T0[k] = fmaf(j02, cm(MV, k, 2), j00 * cm(MV, k, 0));
        T1[k] = fmaf(j12, cm(MV, k, 2), j11 * cm(MV, k, 1));
    }
    const float* cv = g.cov3d;
    const float Sg[9] = {cv[0], cv[1], cv[2], cv[1], cv[3], cv[4], cv[2], cv[4], cv[5]};
    float u0[3], u1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        u0[r] = fmaf(Sg[r * 3 + 2], T0[2], fmaf(Sg[r * 3 + 1], T0[1], Sg[r * 3 + 0] * T0[0]));
        u1[r] = fmaf(Sg[r * 3 + 2], T1[2], fmaf(Sg[r * 3 + 1], T1[1], Sg[r * 3 + 0] * T1[0]));
    }
    const float v00 = fmaf(T0[2], u0[2], fmaf(T0[1], u0[1], T0[0] * u0[0])) + 0.3f;
    const float v01 = fmaf(T0[2], u1[2], fmaf(T0[1], u1[1], T0[0] * u1[0]));
    const float v11 = fmaf(T1[2], u1[2], fmaf(T1[1], u1[1], T1[0] * u1[0])) + 0.3f;
    const float det = fmaf(v00, v11, -(v01 * v01));
    if (!(det > 0.0f)) return false;
    const float idet = 1.0f / det;
    const float A = v11 * idet, B = -v01 * idet, C = v00 * idet;
    // W = -Q G Q
    const float gA = r0.z, hB = 0.5f * r0.w;
    const float m00 = A * gA + B * hB, m01 = A * hB + B * gC, m10 = B * gA + C * hB, m11 = B * hB + C * gC;
    const float w00 = -(m00 * A + m01 * B), w01 = -(m00 * B + m01 * C), w11 = -(m10 * B + m11 * C);
    // dL/dT = 2 W [u0; u1], then to the Jacobian's four entries
    float g0[3], g1[3];
    float gj00 = 0.0f, gj02 = 0.0f, gj11 = 0.0f, gj12 = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g0[k] = 2.0f * (w00 * u0[k] + w01 * u1[k]);
        g1[k] = 2.0f * (w01 * u0[k] + w11 * u1[k]);
        gj00 = k ? gj00 + g0[k] * cm(MV, k, 0) : g0[k] * cm(MV, k, 0);
        gj02 = k ? gj02 + g0[k] * cm(MV, k, 2) : g0[k] * cm(MV, k, 2);
        gj11 = k ? gj11 + g1[k] * cm(MV, k, 1) : g1[k] * cm(MV, k, 1);
        gj12 = k ? gj12 + g1[k] * cm(MV, k, 2) : g1[k] * cm(MV, k, 2);
    }
    const float gid = (gj00 * fx + gj11 * fy) + (2.0f * id) * (gj02 * fxt0 + gj12 * fyt1);
    float gt[4] = {(gj02 * fx) * id2, (gj12 * fy) * id2, gid * id2, 0.0f};
    // ppx = (ph0 / ph3 + 1) W / 2, ppy likewise
    const float iw = 1.0f / ph[3];
    const float gnx = r0.x * (0.5f * (float)ubo.width), gny = r0.y * (0.5f * (float)ubo.height);
    const float gp0 = gnx * iw, gp1 = gny * iw, gp3 = -((gnx * ph[0] + gny * ph[1]) * (iw * iw));
#pragma unroll
    for (int c = 0; c < 4; ++c) gt[c] = gt[c] + ((cm(P, c, 0) * gp0 + cm(P, c, 1) * gp1) + cm(P, c, 3) * gp3);
    if constexpr (DEPTH) gt[2] = gt[2] - row[6];  // depth = -t2
    // t = MV c4, and T's own dependence on MV's 3x3
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) m[c * 4 + r] = gt[r] * c4[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        m[c * 4 + 0] = m[c * 4 + 0] + g0[c] * j00;
        m[c * 4 + 1] = m[c * 4 + 1] + g1[c] * j11;
        m[c * 4 + 2] = m[c * 4 + 2] + (g0[c] * j02 + g1[c] * j12);
    }
    return true;
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
        float m[16];
        if (pose_terms<DEPTH>(ubo, g, rows + 8 * i, m)) {
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
        if (depth)
            hipLaunchKernelGGL(k_pose_partial<true>, dim3(chunks), dim3(kPoseLanes), 0, s, n, ubo, params, rows, partial);
        else
            hipLaunchKernelGGL(k_pose_partial<false>, dim3(chunks), dim3(kPoseLanes), 0, s, n, ubo, params, rows, partial);
    }
    hipLaunchKernelGGL(k_pose_final, dim3(1), dim3(kPoseFinalLanes), 0, s, chunks, partial, out);  // no chunks: 16 x +0
}

}  // namespace gsrt
